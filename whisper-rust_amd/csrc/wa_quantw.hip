// wa_quantw.hip - F32 / F16 values -> ggml weight blocks on the device (wa_quantw_launch.h), the bytes of wa_quantw_rows (wa_quantw.h), which
// are the bytes of the reference's quantize tool.  A code object of its own, built with subnormals kept, correctly rounded divisions and
// square roots, no contraction and no packed F32 instructions: every F32 operation below is the one rounding the host statement has.
//
// 32-value formats (k_quantw32) - bandwidth-bound.  8 lanes own a block, 4 values each from one 16-byte (F32) or 8-byte (F16) load; a
// workgroup of 256 lanes makes 32 blocks.  Minimum, maximum and largest magnitude reduce over the 8 lanes in three DPP steps (two quad
// permutes, one half-row mirror); "the FIRST element that attains it" is a second reduction, of the lowest index whose value equals the
// reduced one, and a third that fetches that element's bits - so the sign of a tied or zero extreme is the scalar loop's.  The 18..34-byte
// blocks are put together in LDS and leave the workgroup as consecutive 16-byte (or 4-byte) stores.
//
// K formats (k_quantw_k45, k_quantw_k6) - search-bound.  One wave owns a super-block, four waves a workgroup; the 256 values (and Q4_K / Q5_K's
// per-element weights) sit in LDS once and every chain reads them as broadcasts in element order.
//   Q4_K / Q5_K: lane = (sub-block j = lane / 8, candidate slot s = lane % 8).  make_qkx2_quants moves `min` with every accepted candidate, so
//   the walk is done in rounds (wa_quantw.h has the argument): the 8 slots of a sub-block evaluate the remaining candidates start + s,
//   start + s + 8, .. on the current min, each stopping at its first one below best_mad; the lowest such `is` of the group (a DPP minimum) is the
//   one the scalar walk accepts; its lane hands (scale, min, mad) to the group and the next round starts behind it.  No candidate's quants are
//   kept: the accepted grid (iscale, min) is, and the quants are recomputed from it in the one case they reach the file (a zero 6-bit scale).
//   Q6_K: lane = (sub-block ib = lane / 4, slot s = lane % 4); the 19 candidates of make_qx_quants are independent, their (sumlx, suml2) go
//   to LDS, and every lane of the group replays the 18 acceptance tests in order.
// The second pass (d / dmin as F16, 6-bit or 8-bit scales, re-quantisation against the rounded scales, nibble / high-bit packing) runs 4
// elements per lane; the 144 / 176 / 210-byte blocks go through LDS like the small ones.
#include "wa_quantw.h"
#include "wa_quantw_launch.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int QW_THREADS = 256;

template <int CTRL> __device__ __forceinline__ uint32_t dpp(uint32_t v) { return (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, CTRL, 0xf, 0xf, true); }
struct op_umax { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a > b ? a : b; } };
struct op_umin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a < b ? a : b; } };
struct op_or   { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return a | b; } };
struct op_fmin { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return __float_as_uint(fminf(__uint_as_float(a), __uint_as_float(b))); } };
struct op_fmax { __device__ uint32_t operator()(uint32_t a, uint32_t b) const { return __float_as_uint(fmaxf(__uint_as_float(a), __uint_as_float(b))); } };
// over the 8 lanes of a group: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror
template <class OP> __device__ __forceinline__ uint32_t red8(uint32_t v, OP op) {
    v = op(v, dpp<0xb1>(v)); v = op(v, dpp<0x4e>(v)); v = op(v, dpp<0x141>(v));
    return v;
}
// lane l of a group <- lane l ^ 4: the half-row mirror (l -> 7 - l), then the quads reversed (quad_perm [3,2,1,0])
__device__ __forceinline__ uint32_t xor4(uint32_t v) { return dpp<0x1b>(dpp<0x141>(v)); }

__device__ __forceinline__ uint32_t f2h_bits(float f) { const _Float16 h = (_Float16) f; uint16_t u; __builtin_memcpy(&u, &h, 2); return u; }      // v_cvt_f16_f32: to nearest even
__device__ __forceinline__ float h2f_val(uint32_t u) { const uint16_t s = (uint16_t) u; _Float16 h; __builtin_memcpy(&h, &s, 2); return (float) h; }   // exact
__device__ __forceinline__ void put32(uint16_t * p, uint32_t w) { p[0] = (uint16_t) w; p[1] = (uint16_t) (w >> 16); }

// 4 consecutive source values of lane `at` (element index of the first one)
template <bool F16> __device__ __forceinline__ void load4(const void * src, size_t at, float v[4]) {
    if (F16) {
        const uint2 u = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint16_t *>(src) + at);
        v[0] = h2f_val(u.x & 0xffffu); v[1] = h2f_val(u.x >> 16); v[2] = h2f_val(u.y & 0xffffu); v[3] = h2f_val(u.y >> 16);
    } else {
        const float4 f = *reinterpret_cast<const float4 *>(reinterpret_cast<const float *>(src) + at);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    }
}

// LDS bytes [0, total) of the workgroup -> dst, consecutive lanes consecutive addresses: 16-byte stores where dst allows, then 4-byte, then one 2-byte
__device__ __forceinline__ void flush(const uint32_t * lds, uint8_t * dst, size_t total) {
    const size_t nq = (reinterpret_cast<uintptr_t>(dst) & 15) == 0 ? total / 16 : 0, nd = total / 4;
    for (size_t i = threadIdx.x; i < nq; i += QW_THREADS) reinterpret_cast<uint4 *>(dst)[i] = reinterpret_cast<const uint4 *>(lds)[i];
    for (size_t i = nq * 4 + threadIdx.x; i < nd; i += QW_THREADS) reinterpret_cast<uint32_t *>(dst)[i] = lds[i];
    if ((total & 2) && threadIdx.x == 0) reinterpret_cast<uint16_t *>(dst)[total / 2 - 1] = reinterpret_cast<const uint16_t *>(lds)[total / 2 - 1];
}

// the first element (lowest index) of the group's 32 whose `hit` is set: its bits
__device__ __forceinline__ uint32_t first_bits(const float v[4], const bool hit[4], int l) {
    uint32_t idx = 32;
#pragma unroll
    for (int j = 3; j >= 0; --j) if (hit[j]) idx = (uint32_t) (4 * l + j);
    idx = red8(idx, op_umin());
    uint32_t b = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (idx == (uint32_t) (4 * l + j)) b = __float_as_uint(v[j]);
    return red8(b, op_or());
}

// ---- 32-value formats --------------------------------------------------------------------------------------------------------------
template <int TYPE, bool F16>
__global__ __launch_bounds__(QW_THREADS) void k_quantw32(const void * __restrict__ src, size_t nblk, uint8_t * __restrict__ dst, uint32_t * __restrict__ flag) {
    constexpr int BS = TYPE == 2 ? 18 : TYPE == 3 ? 20 : TYPE == 6 ? 22 : TYPE == 7 ? 24 : 34;
    __shared__ __attribute__((aligned(16))) uint32_t lds[32 * BS / 4];
    const size_t blk0 = (size_t) blockIdx.x * 32, blk = blk0 + threadIdx.x / 8;
    const int l = threadIdx.x & 7;
    uint16_t * y = reinterpret_cast<uint16_t *>(lds) + (threadIdx.x / 8) * (BS / 2);
    float v[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (blk < nblk) load4<F16>(src, blk * 32 + 4 * (size_t) l, v);      // a block past the end computes on zeros: every lane reaches every DPP step

    uint32_t ab[4], am = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { ab[j] = __float_as_uint(v[j]) & 0x7fffffffu; am = am > ab[j] ? am : ab[j]; }
    am = red8(am, op_umax());
    if (am >= 0x7f800000u && l == 0) *flag = 1u;

    uint32_t q[4];
    if (TYPE == 8) {
        const float d = __uint_as_float(am) / 127, id = d ? 1.0f / d : 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = (uint32_t) wa_qw_trunc(roundf(v[j] * id)) & 0xffu;
        put32(y + 1 + 2 * l, q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24));
        if (l == 0) y[0] = (uint16_t) f2h_bits(d);
    } else {
        float d, id;
        if (TYPE == 2 || TYPE == 6) {
            constexpr int HALF = TYPE == 2 ? 8 : 16, TOP = 2 * HALF - 1;
            bool hit[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) hit[j] = ab[j] == am;
            const uint32_t mb = first_bits(v, hit, l);
            const float max = am == 0 ? 0.0f : __uint_as_float(mb);      // nothing exceeds 0: the scalar loop keeps its +0
            d = max / (float) -HALF; id = d ? 1.0f / d : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { const int a = (int8_t) wa_qw_trunc(v[j] * id + ((float) HALF + 0.5f)); q[j] = (uint32_t) (a < TOP ? a : TOP) & 0xffu; }
            if (l == 0) y[0] = (uint16_t) f2h_bits(d);
        } else {
            constexpr int TOP = TYPE == 3 ? 15 : 31;
            float mn = 3.40282347e+38f, mx = -3.40282347e+38f;
#pragma unroll
            for (int j = 0; j < 4; ++j) { if (v[j] < mn) mn = v[j]; if (v[j] > mx) mx = v[j]; }
            mn = __uint_as_float(red8(__float_as_uint(mn), op_fmin())); mx = __uint_as_float(red8(__float_as_uint(mx), op_fmax()));
            bool hit[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) hit[j] = v[j] == mn;
            mn = __uint_as_float(first_bits(v, hit, l));
#pragma unroll
            for (int j = 0; j < 4; ++j) hit[j] = v[j] == mx;
            mx = __uint_as_float(first_bits(v, hit, l));
            d = (mx - mn) / (float) TOP; id = d ? 1.0f / d : 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int a = wa_qw_trunc((v[j] - mn) * id + 0.5f);
                if (TYPE == 3) { const int a8 = (int8_t) a; q[j] = (uint32_t) (a8 < TOP ? a8 : TOP) & 0xffu; } else q[j] = (uint32_t) a & 0xffu;
            }
            if (l == 0) { y[0] = (uint16_t) f2h_bits(d); y[1] = (uint16_t) f2h_bits(mn); }
        }
        constexpr int QH = TYPE == 6 ? 1 : 2, QS = TYPE == 2 ? 1 : TYPE == 3 ? 2 : TYPE == 6 ? 3 : 4;      // in 16-bit units
        const uint32_t w = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24), nib = w & 0x0f0f0f0fu, other = xor4(nib);
        if (l < 4) put32(y + QS + 2 * l, nib | (other << 4));
        if (TYPE == 6 || TYPE == 7) {
            uint32_t hb = (((q[0] >> 4) & 1u) | (((q[1] >> 4) & 1u) << 1) | (((q[2] >> 4) & 1u) << 2) | (((q[3] >> 4) & 1u) << 3)) << (4 * l);
            hb = red8(hb, op_or());
            if (l == 0) put32(y + QH, hb);
        }
    }
    __syncthreads();
    const size_t live = nblk - blk0 < 32 ? nblk - blk0 : 32;
    flush(lds, dst + blk0 * BS, live * BS);
}

// ---- Q4_K / Q5_K ----------------------------------------------------------------------------------------------------------------------
// one candidate of the group's sub-block (xs, ws: its 32 values and weights in LDS) on the grid (iscale, min); false: D <= 0
__device__ __forceinline__ bool qkx2_candidate(int nmax, const float * xs, const float * ws, float sum_w, float sum_x, float iscale, float min,
                                               float & this_scale, float & this_min, float & mad) {
    float sum_l = 0, sum_l2 = 0, sum_xl = 0;
    for (int i = 0; i < 32; ++i) {
        int q = wa_qw_nearest_int(iscale * (xs[i] - min));
        q = q < 0 ? 0 : q > nmax ? nmax : q;
        const float wl = ws[i] * (float) q;
        sum_l += wl; sum_l2 += wl * (float) q; sum_xl += wl * xs[i];
    }
    const float D = sum_w * sum_l2 - sum_l * sum_l;
    if (!(D > 0)) return false;
    this_scale = (sum_w * sum_xl - sum_x * sum_l) / D;
    this_min   = (sum_l2 * sum_x - sum_l * sum_xl) / D;
    if (this_min > 0) { this_min = 0; this_scale = sum_xl / sum_l2; }
    mad = 0;
    for (int i = 0; i < 32; ++i) {
        int q = wa_qw_nearest_int(iscale * (xs[i] - min));
        q = q < 0 ? 0 : q > nmax ? nmax : q;
        float diff = this_scale * (float) q + this_min - xs[i];
        diff = diff * diff;
        mad += ws[i] * diff;
    }
    return true;
}

template <int TYPE, bool F16>
__global__ __launch_bounds__(QW_THREADS) void k_quantw_k45(const void * __restrict__ src, size_t nblk, uint8_t * __restrict__ dst, uint32_t * __restrict__ flag) {
    constexpr int BS = TYPE == 12 ? 144 : 176, NMAX = TYPE == 12 ? 15 : 31, NSTEP = TYPE == 12 ? 20 : 15;
    constexpr float RMIN = TYPE == 12 ? -1.f : -0.5f, RDELTA = 0.1f;
    __shared__ __attribute__((aligned(16))) float xs_all[4][256];
    __shared__ __attribute__((aligned(16))) float ws_all[4][256];
    __shared__ __attribute__((aligned(16))) uint32_t L_all[4][64];
    __shared__ __attribute__((aligned(16))) uint32_t out_all[4 * BS / 4];
    __shared__ float sm_all[4][16];
    const int wv = threadIdx.x / 64, t = threadIdx.x & 63, j = t >> 3, s = t & 7;
    const size_t blk0 = (size_t) blockIdx.x * 4, blk = blk0 + wv;
    float * xs = xs_all[wv], * ws = ws_all[wv], * sm = sm_all[wv];
    uint16_t * out = reinterpret_cast<uint16_t *>(out_all) + wv * (BS / 2);

    float v[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (blk < nblk) load4<F16>(src, blk * 256 + 4 * (size_t) t, v);      // a wave past the end works on zeros and reaches every barrier
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) { xs[4 * t + k] = v[k]; bad |= !wa_qw_finite(v[k]); }
    if (bad) *flag = 1u;
    __syncthreads();

    const float * xj = xs + 32 * j, * wj = ws + 32 * j;
    {   // the weights of sub-block j: every lane of the group runs the same chain, lane s writes elements 4 s .. 4 s + 3
        float sum_x2 = 0;
        for (int i = 0; i < 32; ++i) sum_x2 += xj[i] * xj[i];
        const float av_x = sqrtf(sum_x2 / 32);
#pragma unroll
        for (int k = 0; k < 4; ++k) ws[4 * t + k] = av_x + fabsf(v[k]);
    }
    __syncthreads();

    float min = xj[0], max = xj[0], sum_w = wj[0], sum_x = sum_w * xj[0];
    for (int i = 1; i < 32; ++i) {
        if (xj[i] < min) min = xj[i];
        if (xj[i] > max) max = xj[i];
        sum_w += wj[i]; sum_x += wj[i] * xj[i];
    }
    if (min > 0) min = 0;
    const bool flat = max == min;
    float scale = 0.f, best_mad = 0, win_iscale = 0.f, win_min = min;
    if (!flat) {
        win_iscale = (float) NMAX / (max - min); scale = 1 / win_iscale;
        for (int i = 0; i < 32; ++i) {
            int q = wa_qw_nearest_int(win_iscale * (xj[i] - min));
            q = q < 0 ? 0 : q > NMAX ? NMAX : q;
            float diff = scale * (float) q + min - xj[i];
            diff = diff * diff;
            best_mad += wj[i] * diff;
        }
    }
    // the rounds: one acceptance of the scalar walk each
    int start = 0;
    bool active = !flat;
    while (__ballot(active) != 0) {
        uint32_t c_is = 0x7fffffffu;
        float c_scale = 0, c_min = 0, c_mad = 0, c_iscale = 0;
        if (active) {
            for (int is = start + s; is <= NSTEP; is += 8) {
                const float iscale = (RMIN + RDELTA * (float) is + (float) NMAX) / (max - min);
                float ts, tm, mad;
                if (qkx2_candidate(NMAX, xj, wj, sum_w, sum_x, iscale, min, ts, tm, mad) && mad < best_mad) {
                    c_is = (uint32_t) is; c_scale = ts; c_min = tm; c_mad = mad; c_iscale = iscale;
                    break;
                }
            }
        }
        const uint32_t g_is = red8(c_is, op_umin());
        const int from = (t & ~7) | (int) ((g_is - (uint32_t) start) & 7u);      // the slot that holds candidate g_is
        const float a_scale = __shfl(c_scale, from), a_min = __shfl(c_min, from), a_mad = __shfl(c_mad, from), a_iscale = __shfl(c_iscale, from);
        if (active) {
            if (g_is == 0x7fffffffu) active = false;
            else {
                win_iscale = a_iscale; win_min = min;
                scale = a_scale; min = a_min; best_mad = a_mad;
                start = (int) g_is + 1;
                active = start <= NSTEP;
            }
        }
    }
    if (s == 0) { sm[j] = scale; sm[8 + j] = -min; }
    __syncthreads();

    float max_scale = 0, max_min = 0;
    for (int k = 0; k < 8; ++k) { if (sm[k] > max_scale) max_scale = sm[k]; if (sm[8 + k] > max_min) max_min = sm[8 + k]; }
    const float inv_scale = max_scale > 0 ? 63.f / max_scale : 0.f, inv_min = max_min > 0 ? 63.f / max_min : 0.f;
    const uint32_t dh = f2h_bits(max_scale / 63.f), mh = f2h_bits(max_min / 63.f);
    auto six = [&](float inv, float val) { const uint32_t u = (uint32_t) wa_qw_nearest_int(inv * val) & 0xffu; return u < 63u ? u : 63u; };
    if (t == 0) {      // d, dmin and the 12 scale bytes
        uint32_t b[12];
        for (int k = 0; k < 12; ++k) b[k] = 0;
        for (int k = 0; k < 8; ++k) {
            const uint32_t ls = six(inv_scale, sm[k]), lm = six(inv_min, sm[8 + k]);
            if (k < 4) { b[k] |= ls; b[k + 4] |= lm; }
            else { b[k + 4] = (ls & 15u) | ((lm & 15u) << 4); b[k - 4] |= (ls >> 4) << 6; b[k] |= (lm >> 4) << 6; }
        }
        out[0] = (uint16_t) dh; out[1] = (uint16_t) mh;
        for (int k = 0; k < 6; ++k) out[2 + k] = (uint16_t) (b[2 * k] | (b[2 * k + 1] << 8));
    }
    {   // elements 4 t .. 4 t + 3 (sub-block j) against the rounded scales
        const float d = h2f_val(dh) * (float) six(inv_scale, sm[j]), dm = h2f_val(mh) * (float) six(inv_min, sm[8 + j]);
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q = 0;
            if (d != 0) q = wa_qw_nearest_int((v[k] + dm) / d);
            else if (!flat) q = wa_qw_nearest_int(win_iscale * (v[k] - win_min));      // the search's own quants stay
            q = q < 0 ? 0 : q > NMAX ? NMAX : q;
            w |= (uint32_t) q << (8 * k);
        }
        L_all[wv][t] = w;
    }
    __syncthreads();
    if (t < 32) {      // qs: bytes 4 t .. 4 t + 3 of the 128
        const int g = t >> 3, l0 = t & 7;
        const uint32_t a = L_all[wv][16 * g + l0], b = L_all[wv][16 * g + 8 + l0];
        put32(out + (TYPE == 12 ? 8 : 24) + 2 * t, (a & 0x0f0f0f0fu) | ((b & 0x0f0f0f0fu) << 4));
    } else if (TYPE == 13 && t < 40) {      // qh: bytes 4 u .. 4 u + 3 of the 32
        const int u = t - 32;
        uint32_t h = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) h |= (((L_all[wv][16 * g + u] >> 4) & 0x01010101u) << (2 * g)) | (((L_all[wv][16 * g + 8 + u] >> 4) & 0x01010101u) << (2 * g + 1));
        put32(out + 8 + 2 * u, h);
    }
    __syncthreads();
    const size_t live = nblk - blk0 < 4 ? nblk - blk0 : 4;
    flush(out_all, dst + blk0 * BS, live * BS);
}

// ---- Q6_K ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float qx_iscale(int k, float max) {      // candidate k = 0: the first grid; 1..18: is = -9..-1, 1..9
    if (k == 0) return -32.f / max;
    const int is = k <= 9 ? k - 10 : k - 9;
    return -(32.f + 0.1f * (float) is) / max;
}
__device__ __forceinline__ int qx_quant(float iscale, float x) { const int l = wa_qw_nearest_int(iscale * x); return l < -32 ? -32 : l > 31 ? 31 : l; }

template <bool F16>
__global__ __launch_bounds__(QW_THREADS) void k_quantw_k6(const void * __restrict__ src, size_t nblk, uint8_t * __restrict__ dst, uint32_t * __restrict__ flag) {
    constexpr int BS = 210;
    __shared__ __attribute__((aligned(16))) float xs_all[4][256];
    __shared__ float cs_all[4][16][19][2];
    __shared__ float sm_all[4][16];
    __shared__ __attribute__((aligned(16))) uint32_t L_all[4][64];
    __shared__ __attribute__((aligned(16))) uint32_t out_all[4 * BS / 4];
    const int wv = threadIdx.x / 64, t = threadIdx.x & 63, ib = t >> 2, s = t & 3;
    const size_t blk0 = (size_t) blockIdx.x * 4, blk = blk0 + wv;
    float * xs = xs_all[wv], * sm = sm_all[wv];
    uint16_t * out = reinterpret_cast<uint16_t *>(out_all) + wv * (BS / 2);

    float v[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (blk < nblk) load4<F16>(src, blk * 256 + 4 * (size_t) t, v);
    bool bad = false;
#pragma unroll
    for (int k = 0; k < 4; ++k) { xs[4 * t + k] = v[k]; bad |= !wa_qw_finite(v[k]); }
    if (bad) *flag = 1u;
    __syncthreads();

    const float * xb = xs + 16 * ib;
    float max = 0, amax = 0;
    for (int i = 0; i < 16; ++i) { const float ax = fabsf(xb[i]); if (ax > amax) { amax = ax; max = xb[i]; } }
    const bool zero = amax < WA_QW_GROUP_MAX_EPS;
    if (!zero) {
        for (int k = s; k < 19; k += 4) {
            const float iscale = qx_iscale(k, max);
            float sumlx = 0, suml2 = 0;
            for (int i = 0; i < 16; ++i) {
                const float l = (float) qx_quant(iscale, xb[i]), w = xb[i] * xb[i];
                sumlx += w * xb[i] * l;
                suml2 += w * l * l;
            }
            cs_all[wv][ib][k][0] = sumlx; cs_all[wv][ib][k][1] = suml2;
        }
    }
    __syncthreads();
    float scale = 0.f;
    int win = 0;
    if (!zero) {      // the ordered replay
        const float sumlx0 = cs_all[wv][ib][0][0], suml20 = cs_all[wv][ib][0][1];
        scale = suml20 ? sumlx0 / suml20 : 0.0f;
        float best = scale * sumlx0;
        for (int k = 1; k < 19; ++k) {
            const float sumlx = cs_all[wv][ib][k][0], suml2 = cs_all[wv][ib][k][1];
            if (suml2 > 0 && sumlx * sumlx > best * suml2) { scale = sumlx / suml2; best = scale * sumlx; win = k; }
        }
    }
    if (s == 0) sm[ib] = scale;
    __syncthreads();

    float max_scale = 0, max_abs_scale = 0;
    for (int k = 0; k < 16; ++k) { const float a = fabsf(sm[k]); if (a > max_abs_scale) { max_abs_scale = a; max_scale = sm[k]; } }
    const bool empty = max_abs_scale < WA_QW_GROUP_MAX_EPS;      // the whole block is zero bytes
    const float iscale_g = empty ? 0.f : -128.f / max_scale;
    const uint32_t dh = empty ? 0u : f2h_bits(1 / iscale_g);
    auto sc8 = [&](int k) { const int q = wa_qw_nearest_int(iscale_g * sm[k]); return empty ? 0 : q < 127 ? q : 127; };
    {
        const float d = h2f_val(dh) * (float) (int8_t) sc8(ib);
        uint32_t w = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            int q = 0;
            if (d != 0) q = 32 + qx_quant(1.0f, v[k] / d);
            else if (!zero) q = 32 + qx_quant(qx_iscale(win, max), v[k]);      // the search's own quants stay
            w |= (uint32_t) q << (8 * k);
        }
        L_all[wv][t] = empty ? 0u : w;
    }
    __syncthreads();
    const uint32_t * L = L_all[wv];
    if (t < 32) {      // ql: bytes 4 t .. 4 t + 3 of the 128
        const int h = t >> 4, p = (t >> 3) & 1, l0 = t & 7;
        const uint32_t a = L[32 * h + 8 * p + l0], c = L[32 * h + 16 + 8 * p + l0];
        put32(out + 2 * t, (a & 0x0f0f0f0fu) | ((c & 0x0f0f0f0fu) << 4));
    } else if (t < 48) {      // qh: bytes 4 u .. 4 u + 3 of the 64
        const int u = t - 32, h = u >> 3, l0 = u & 7;
        uint32_t w = 0;
#pragma unroll
        for (int g = 0; g < 4; ++g) w |= ((L[32 * h + 8 * g + l0] >> 4) & 0x03030303u) << (2 * g);
        put32(out + 64 + 2 * u, w);
    } else if (t < 52) {      // the 16 scales
        const int u = t - 48;
        uint32_t w = 0;
        for (int k = 0; k < 4; ++k) w |= ((uint32_t) sc8(4 * u + k) & 0xffu) << (8 * k);
        put32(out + 96 + 2 * u, w);
    } else if (t == 52) out[104] = (uint16_t) dh;
    __syncthreads();
    const size_t live = nblk - blk0 < 4 ? nblk - blk0 : 4;
    flush(out_all, dst + blk0 * BS, live * BS);
}

template <bool F16> int launch(hipStream_t st, int type, const void * src, size_t n, uint8_t * dst, uint32_t * flag) {
    const dim3 g32((unsigned) ((n + 31) / 32)), gk((unsigned) ((n + 3) / 4)), b(QW_THREADS);
    switch (type) {
        case 2:  hipLaunchKernelGGL((k_quantw32<2, F16>), g32, b, 0, st, src, n, dst, flag); break;
        case 3:  hipLaunchKernelGGL((k_quantw32<3, F16>), g32, b, 0, st, src, n, dst, flag); break;
        case 6:  hipLaunchKernelGGL((k_quantw32<6, F16>), g32, b, 0, st, src, n, dst, flag); break;
        case 7:  hipLaunchKernelGGL((k_quantw32<7, F16>), g32, b, 0, st, src, n, dst, flag); break;
        case 8:  hipLaunchKernelGGL((k_quantw32<8, F16>), g32, b, 0, st, src, n, dst, flag); break;
        case 12: hipLaunchKernelGGL((k_quantw_k45<12, F16>), gk, b, 0, st, src, n, dst, flag); break;
        case 13: hipLaunchKernelGGL((k_quantw_k45<13, F16>), gk, b, 0, st, src, n, dst, flag); break;
        case 14: hipLaunchKernelGGL((k_quantw_k6<F16>), gk, b, 0, st, src, n, dst, flag); break;
        default: return (int) hipErrorInvalidValue;
    }
    return (int) hipGetLastError();
}

} // namespace

int wa_launch_quantw(void * stream, int type, const void * src, int src_is_f16, size_t nblocks, uint8_t * dst, uint32_t * flag) {
    if (!wa_qw_block_values(type) || !src || !dst || !flag || (reinterpret_cast<uintptr_t>(src) & 15) != 0 || (reinterpret_cast<uintptr_t>(dst) & 3) != 0 ||
        nblocks > (size_t) 0x7fffffff) return (int) hipErrorInvalidValue;
    if (nblocks == 0) return 0;
    hipStream_t st = (hipStream_t) stream;
    return src_is_f16 ? launch<true>(st, type, src, nblocks, dst, flag) : launch<false>(st, type, src, nblocks, dst, flag);
}

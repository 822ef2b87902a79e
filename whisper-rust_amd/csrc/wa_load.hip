// wa_load.hip - the model loader's unpack kernels (wa_load.h): raw tensor bytes of a run of whole rows, as the file holds them, in a device
// staging buffer -> the arena arrays the product kernels read.  Integer work and the exact F16 -> F32 widening only, so the results are the
// bits the host functions give (wa_q32_unpack_rows, wa_qk_unpack_rows, wa_conv_reorder_rows) - the kernels restate THEM, four quants at a
// time in one 32-bit word.  A code object of its own.
//
// Shape: one thread per 16 (32-value formats: one lane's bytes of four blocks) or 32 (K formats: one lane's bytes of one block) contiguous
// output bytes, written by 16-byte stores; consecutive threads write consecutive addresses.  The reads are 2-byte loads - a 22-, 34-, 110- or
// 210-byte block is aligned to no more - of blocks a few hundred bytes apart, which the caches serve: every byte of the staging buffer is
// read by the eight lanes of its block back to back.  No LDS, no scratch.
#include "wa_load.h"
#include "wa_quantk.h"

#include <hip/hip_runtime.h>

namespace {

constexpr int LD_THREADS = 256;

__device__ __forceinline__ uint32_t ld16(const uint8_t * p) { return *reinterpret_cast<const uint16_t *>(p); }
__device__ __forceinline__ uint32_t ld32(const uint8_t * p) { return ld16(p) | (ld16(p + 2) << 16); }

// IEEE half -> float in integer arithmetic (wa_q1_h2f / wa_qk_h2f): exact, subnormals included, a NaN keeps its payload
__device__ __forceinline__ float h2f_bits(uint32_t h) {
    const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    uint32_t u;
    if (e == 31u) u = sign | 0x7f800000u | (m << 13);
    else if (e != 0u) u = sign | ((e + 112u) << 23) | (m << 13);
    else if (m == 0u) u = sign;
    else { const int p = 31 - __clz((int) m); u = sign | ((uint32_t) (p + 103) << 23) | ((m << (23 - p)) & 0x7fffffu); }      // m 2^-24 = 1.x 2^(p - 24)
    return __uint_as_float(u);
}

// ---- 32-value formats --------------------------------------------------------------------------------------------------------------
template <int TYPE> __device__ __forceinline__ constexpr int q32_bytes() { return TYPE == 6 ? 22 : TYPE == 8 ? 34 : TYPE == 3 ? 20 : 24; }

// elements 4 l .. 4 l + 3 of a block as four bytes
template <int TYPE> __device__ __forceinline__ uint32_t q32_word(const uint8_t * blk, int l) {
    if (TYPE == 8) return ld32(blk + 2 + 4 * l);
    const int qo = TYPE == 6 ? 6 : TYPE == 3 ? 4 : 8;                       // where qs[16] starts
    const uint32_t w = ld32(blk + qo + 4 * (l & 3));
    const uint32_t nib = (l < 4 ? w : w >> 4) & 0x0f0f0f0fu;               // elements 0..15: low nibbles, 16..31: high nibbles
    if (TYPE == 3) return nib;
    const uint32_t bits = (ld32(blk + (TYPE == 6 ? 2 : 4)) >> (4 * l)) & 0xfu;      // bit e of qh: the fifth bit of element e
    const uint32_t v = nib | ((bits & 1u) << 4) | ((bits & 2u) << 11) | ((bits & 4u) << 18) | ((bits & 8u) << 25);
    if (TYPE == 7) return v;
    const uint32_t r = v ^ 0x10101010u;                                     // Q5_0: minus 16 in every byte (16..31 -> 0..15, 0..15 -> 0xf0..0xff)
    return r | (((r >> 4) & 0x01010101u) * 0xe0u);
}

// VEC: nb % 4 == 0, one thread = lane l of blocks 4 bq .. 4 bq + 3, one 16-byte store; else one thread = lane l of one block
template <int TYPE, bool VEC>
__global__ __launch_bounds__(LD_THREADS) void k_load_q32(const uint8_t * __restrict__ src, size_t rows, size_t nb, int8_t * __restrict__ qs,
                                                         float * __restrict__ qd, float * __restrict__ qm) {
    constexpr int BS = q32_bytes<TYPE>(), NBLK = VEC ? 4 : 1;
    constexpr bool MIN = TYPE == 3 || TYPE == 7;
    const size_t per_lane = nb / NBLK, t = (size_t) blockIdx.x * LD_THREADS + threadIdx.x;
    if (t >= rows * 8 * per_lane) return;
    const size_t bq = t % per_lane, row = t / (8 * per_lane);
    const int l = (int) ((t / per_lane) % 8);
    const uint8_t * blk = src + (row * nb + bq * NBLK) * BS;
    uint32_t w[NBLK];
#pragma unroll
    for (int i = 0; i < NBLK; ++i) w[i] = q32_word<TYPE>(blk + i * BS, l);
    int8_t * out = qs + ((row * 8 + l) * nb + bq * NBLK) * 4;
    if (VEC) *reinterpret_cast<uint4 *>(out) = make_uint4(w[0], w[NBLK > 1 ? 1 : 0], w[NBLK > 1 ? 2 : 0], w[NBLK > 1 ? 3 : 0]);
    else *reinterpret_cast<uint32_t *>(out) = w[0];
    if (l == 0 || (MIN && l == 1)) {                                        // lane 0: the scales, lane 1: the minimums
        float f[NBLK];
#pragma unroll
        for (int i = 0; i < NBLK; ++i) f[i] = h2f_bits(ld16(blk + i * BS + 2 * l));
        float * dst = (l == 0 ? qd : qm) + row * nb + bq * NBLK;
        if (VEC) *reinterpret_cast<float4 *>(dst) = make_float4(f[0], f[NBLK > 1 ? 1 : 0], f[NBLK > 1 ? 2 : 0], f[NBLK > 1 ? 3 : 0]);
        else *dst = f[0];
    }
}

// ---- K formats ---------------------------------------------------------------------------------------------------------------------
// elements 32 g + 4 l .. + 3 of a block for g = 0..7, as eight words
template <int TYPE> __device__ __forceinline__ void qk_words(const uint8_t * blk, int l, uint32_t out[8]) {
    if (TYPE == WA_TYPE_Q6_K) {
#pragma unroll
        for (int hf = 0; hf < 2; ++hf) {
            const uint32_t la = ld32(blk + 64 * hf + 4 * l), lb = ld32(blk + 64 * hf + 32 + 4 * l), h = ld32(blk + 128 + 32 * hf + 4 * l);
            out[4 * hf + 0] = (la & 0x0f0f0f0fu)        | ((h         & 0x03030303u) << 4);
            out[4 * hf + 1] = (lb & 0x0f0f0f0fu)        | (((h >> 2)  & 0x03030303u) << 4);
            out[4 * hf + 2] = ((la >> 4) & 0x0f0f0f0fu) | (((h >> 4)  & 0x03030303u) << 4);
            out[4 * hf + 3] = ((lb >> 4) & 0x0f0f0f0fu) | (((h >> 6)  & 0x03030303u) << 4);
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) { const uint32_t r = out[g] ^ 0x20202020u; out[g] = r | (((r >> 5) & 0x01010101u) * 0xc0u); }      // minus 32 in every byte
    } else if (TYPE == WA_TYPE_Q3_K) {
        const uint32_t hm = ld32(blk + 4 * l);
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const uint32_t w = ld32(blk + 32 + 32 * n + 4 * l);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t t = ((w >> (2 * j)) & 0x03030303u) | (((hm >> (4 * n + j)) & 0x01010101u) << 2);      // 0..7; the value is t - 4
                const uint32_t r = t ^ 0x04040404u;
                out[4 * n + j] = r | (((r >> 2) & 0x01010101u) * 0xf8u);
            }
        }
    } else if (TYPE == WA_TYPE_Q2_K) {
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const uint32_t w = ld32(blk + 16 + 32 * n + 4 * l);
#pragma unroll
            for (int j = 0; j < 4; ++j) out[4 * n + j] = (w >> (2 * j)) & 0x03030303u;
        }
    } else {
        const uint32_t qh = ld32(blk + 16 + 4 * l);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = ld32(blk + 48 + 32 * k + 4 * l);
            out[2 * k]     = (w & 0x0f0f0f0fu)        | (((qh >> (2 * k))     & 0x01010101u) << 4);
            out[2 * k + 1] = ((w >> 4) & 0x0f0f0f0fu) | (((qh >> (2 * k + 1)) & 0x01010101u) << 4);
        }
    }
}

// the 16 scale bytes of a block in the order wa_qk_unpack gives them, as four words
template <int TYPE> __device__ __forceinline__ void qk_scales(const uint8_t * blk, uint32_t sc[4]) {
    sc[0] = sc[1] = sc[2] = sc[3] = 0;
    auto put = [&](int at, uint32_t v) { sc[at >> 2] |= (v & 0xffu) << (8 * (at & 3)); };
    if (TYPE == WA_TYPE_Q6_K || TYPE == WA_TYPE_Q2_K) {
        const uint8_t * s = blk + (TYPE == WA_TYPE_Q6_K ? 192 : 0);
#pragma unroll
        for (int g = 0; g < 8; ++g) { const uint32_t p = ld16(s + 2 * g); put(g, p); put(8 + g, p >> 8); }
    } else if (TYPE == WA_TYPE_Q3_K) {
        const uint8_t * s = blk + 96;
        uint32_t b[12];
#pragma unroll
        for (int i = 0; i < 6; ++i) { const uint32_t p = ld16(s + 2 * i); b[2 * i] = p & 0xffu; b[2 * i + 1] = p >> 8; }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const uint32_t lo = k < 8 ? b[k] & 0xfu : b[k - 8] >> 4, hi = (b[8 + (k & 3)] >> (2 * (k >> 2))) & 3u;
            put(8 * (k & 1) + (k >> 1), (lo | (hi << 4)) - 32u);
        }
    } else {
        const uint8_t * s = blk + 4;
        uint32_t b[12];
#pragma unroll
        for (int i = 0; i < 6; ++i) { const uint32_t p = ld16(s + 2 * i); b[2 * i] = p & 0xffu; b[2 * i + 1] = p >> 8; }
#pragma unroll
        for (int j = 0; j < 8; ++j) {                                       // get_scale_min_k4
            if (j < 4) { put(j, b[j] & 63u); put(8 + j, b[j + 4] & 63u); }
            else       { put(j, (b[j + 4] & 0xfu) | ((b[j - 4] >> 6) << 4)); put(8 + j, (b[j + 4] >> 4) | ((b[j] >> 6) << 4)); }
        }
    }
}

// one thread = lane l of one block: 32 contiguous quant bytes, two 16-byte stores; lane 0 adds the block's scale bytes, lane 1 its d (and dmin)
template <int TYPE>
__global__ __launch_bounds__(LD_THREADS) void k_load_qk(const uint8_t * __restrict__ src, size_t rows, size_t nb, int8_t * __restrict__ qs,
                                                        int8_t * __restrict__ qsc, float * __restrict__ qd, float * __restrict__ qm) {
    constexpr int BS = TYPE == WA_TYPE_Q5_K ? WA_Q5_K_BYTES : TYPE == WA_TYPE_Q6_K ? WA_Q6_K_BYTES : TYPE == WA_TYPE_Q2_K ? WA_Q2_K_BYTES : WA_Q3_K_BYTES;
    constexpr int D_AT = TYPE == WA_TYPE_Q6_K ? 208 : TYPE == WA_TYPE_Q3_K ? 108 : TYPE == WA_TYPE_Q2_K ? 80 : 0;
    constexpr bool MIN = TYPE == WA_TYPE_Q5_K || TYPE == WA_TYPE_Q2_K;
    const size_t t = (size_t) blockIdx.x * LD_THREADS + threadIdx.x;
    if (t >= rows * 8 * nb) return;
    const size_t b = t % nb, row = t / (8 * nb);
    const int l = (int) ((t / nb) % 8);
    const uint8_t * blk = src + (row * nb + b) * BS;
    uint32_t w[8];
    qk_words<TYPE>(blk, l, w);
    uint4 * out = reinterpret_cast<uint4 *>(qs + ((row * 8 + l) * nb + b) * 32);
    out[0] = make_uint4(w[0], w[1], w[2], w[3]);
    out[1] = make_uint4(w[4], w[5], w[6], w[7]);
    if (l == 0) {
        uint32_t sc[4];
        qk_scales<TYPE>(blk, sc);
        *reinterpret_cast<uint4 *>(qsc + (row * nb + b) * 16) = make_uint4(sc[0], sc[1], sc[2], sc[3]);
    } else if (l == 1) {
        qd[row * nb + b] = h2f_bits(ld16(blk + D_AT));
        if (MIN) qm[row * nb + b] = h2f_bits(ld16(blk + D_AT + 2));
    }
}

// ---- conv weights ------------------------------------------------------------------------------------------------------------------
// IC % 8 == 0, ld % 8 == 0, 16-byte aligned pointers: one thread = eight input channels of one output channel, 48 contiguous bytes in,
// the same 48 bytes to the copy, three 16-byte stores (one per tap k) to the re-ordered rows
__global__ __launch_bounds__(LD_THREADS) void k_load_conv8(const uint16_t * __restrict__ src, size_t rows, int IC, int ld, uint16_t * __restrict__ dst,
                                                           uint16_t * __restrict__ copy) {
    const size_t per_row = (size_t) IC / 8, t = (size_t) blockIdx.x * LD_THREADS + threadIdx.x;
    if (t >= rows * per_row) return;
    const size_t oc = t / per_row, ic0 = (t % per_row) * 8;
    const uint4 * in = reinterpret_cast<const uint4 *>(src + (oc * IC + ic0) * 3);
    const uint4 a = in[0], b = in[1], c = in[2];
    uint4 * cp = reinterpret_cast<uint4 *>(copy + (oc * IC + ic0) * 3);
    cp[0] = a; cp[1] = b; cp[2] = c;
    const uint32_t w[12] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
    auto h = [&](int i) { return (w[i >> 1] >> (16 * (i & 1))) & 0xffffu; };      // half i of the 24: input channel i / 3, tap i % 3
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint4 o = make_uint4(h(k) | (h(3 + k) << 16), h(6 + k) | (h(9 + k) << 16), h(12 + k) | (h(15 + k) << 16), h(18 + k) | (h(21 + k) << 16));
        *reinterpret_cast<uint4 *>(dst + oc * (size_t) ld + (size_t) k * IC + ic0) = o;
    }
}
// any other shape: one thread per element
__global__ __launch_bounds__(LD_THREADS) void k_load_conv1(const uint16_t * __restrict__ src, size_t rows, int IC, int ld, uint16_t * __restrict__ dst,
                                                           uint16_t * __restrict__ copy) {
    const size_t t = (size_t) blockIdx.x * LD_THREADS + threadIdx.x;
    if (t >= rows * (size_t) IC * 3) return;
    const size_t k = t % 3, ic = (t / 3) % (size_t) IC, oc = t / (3 * (size_t) IC);
    const uint16_t v = src[t];
    copy[t] = v;
    dst[oc * (size_t) ld + k * (size_t) IC + ic] = v;
}

inline unsigned blocks_for(size_t threads) { return (unsigned) ((threads + LD_THREADS - 1) / LD_THREADS); }
inline bool aligned16(const void * p) { return ((uintptr_t) p & 15u) == 0; }
constexpr size_t MAX_THREADS = (size_t) 1 << 38;      // 2^30 workgroups of 256: a launch beyond it is refused, not truncated

template <int TYPE>
int launch_q32(hipStream_t st, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, float * qd, float * qm) {
    const bool vec = nb % 4 == 0 && aligned16(qs) && aligned16(qd) && (!qm || aligned16(qm));
    const size_t threads = rows * 8 * (vec ? nb / 4 : nb);
    if (vec) k_load_q32<TYPE, true><<<blocks_for(threads), LD_THREADS, 0, st>>>(src, rows, nb, qs, qd, qm);
    else     k_load_q32<TYPE, false><<<blocks_for(threads), LD_THREADS, 0, st>>>(src, rows, nb, qs, qd, qm);
    return (int) hipGetLastError();
}

} // namespace

int wa_launch_load_q32(void * stream, int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, float * qd, float * qm) {
    hipStream_t st = (hipStream_t) stream;
    const bool has_min = type == 3 || type == 7;
    if (!src || !qs || !qd || has_min != (qm != nullptr) || ((uintptr_t) src & 1u) || ((uintptr_t) qs & 3u)) return (int) hipErrorInvalidValue;
    if (rows == 0 || nb == 0) return 0;
    if (rows > MAX_THREADS / 8 / nb) return (int) hipErrorInvalidValue;
    switch (type) {
        case 6: return launch_q32<6>(st, src, rows, nb, qs, qd, qm);
        case 8: return launch_q32<8>(st, src, rows, nb, qs, qd, qm);
        case 3: return launch_q32<3>(st, src, rows, nb, qs, qd, qm);
        case 7: return launch_q32<7>(st, src, rows, nb, qs, qd, qm);
    }
    return (int) hipErrorInvalidValue;
}

int wa_launch_load_qk(void * stream, int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, int8_t * qsc, float * qd, float * qm) {
    hipStream_t st = (hipStream_t) stream;
    if (!src || !qs || !qsc || !qd || wa_qk_has_min(type) != (qm != nullptr) || ((uintptr_t) src & 1u) || !aligned16(qs) || !aligned16(qsc)) return (int) hipErrorInvalidValue;
    if (rows == 0 || nb == 0) return 0;
    if (rows > MAX_THREADS / 8 / nb) return (int) hipErrorInvalidValue;
    const unsigned g = blocks_for(rows * 8 * nb);
    switch (type) {
        case WA_TYPE_Q2_K: k_load_qk<WA_TYPE_Q2_K><<<g, LD_THREADS, 0, st>>>(src, rows, nb, qs, qsc, qd, qm); break;
        case WA_TYPE_Q3_K: k_load_qk<WA_TYPE_Q3_K><<<g, LD_THREADS, 0, st>>>(src, rows, nb, qs, qsc, qd, qm); break;
        case WA_TYPE_Q5_K: k_load_qk<WA_TYPE_Q5_K><<<g, LD_THREADS, 0, st>>>(src, rows, nb, qs, qsc, qd, qm); break;
        case WA_TYPE_Q6_K: k_load_qk<WA_TYPE_Q6_K><<<g, LD_THREADS, 0, st>>>(src, rows, nb, qs, qsc, qd, qm); break;
        default: return (int) hipErrorInvalidValue;
    }
    return (int) hipGetLastError();
}

int wa_launch_load_conv(void * stream, const uint16_t * src, size_t rows, int IC, int ld, uint16_t * dst, uint16_t * copy) {
    hipStream_t st = (hipStream_t) stream;
    if (!src || !dst || !copy || IC <= 0 || ld < 3 * IC) return (int) hipErrorInvalidValue;
    if (rows == 0) return 0;
    if (rows > MAX_THREADS / 3 / (size_t) IC) return (int) hipErrorInvalidValue;
    if (IC % 8 == 0 && ld % 8 == 0 && aligned16(src) && aligned16(dst) && aligned16(copy))
        k_load_conv8<<<blocks_for(rows * (size_t) (IC / 8)), LD_THREADS, 0, st>>>(src, rows, IC, ld, dst, copy);
    else
        k_load_conv1<<<blocks_for(rows * (size_t) IC * 3), LD_THREADS, 0, st>>>(src, rows, IC, ld, dst, copy);
    return (int) hipGetLastError();
}

// wa_rows_q8k_dev.h - the Q8_K operand rows of the several-rows decode step's K-format kernels (wa_rows.hip: k_decode_rows_k_np*, _k5_np*, _k2_np*,
// _q4k_np*): how such a row lies in LDS, and the quantiser that writes one block of it from a wave's registers - in both of the reference's rules.
// A header of its own so that tests/native/rows_q4k_quant.hip can launch the quantiser in isolation.
//
// An operand row: quants in the order of the K-format weight rows - lane u's 32 bytes of a block are [group 0..7][4], two 16-byte reads, the eight
// lanes' runs an odd number of 16-byte cells apart (mk_ls), so the reads of a step fall on disjoint banks -, then (sums) the blocks' bsums, then its
// F32 d per block.
#pragma once
#include "wa_one_launch_dev.h"

__host__ __device__ __forceinline__ int mk_ls(int nbk) { return 32 * nbk + 16; }         // bytes between the lanes' runs of an operand row
// (sums: the formats with a minimum term, Q5_K and Q2_K - k_decode_rows_k5_np* / _k2_np* -, read the operand's block sums.  Their rows hold, between the
//  quants and the d, the 16 int16 sums of 16 elements of every block, as block_q8_K::bsums orders them - ONE layout for both: Q2_K's lane u reads sums 2 u
//  and 2 u + 1 as dword u of the block, Q5_K's chain the same dwords, four to a 16-byte read, and adds the halves; pair sums alone would have saved 16
//  bytes a block and served Q5_K only.  In front of the d, so that they start on a 16-byte boundary whatever the block count.  Q4_K reads them as Q5_K.)
__host__ __device__ __forceinline__ size_t mk_xd_off(int nbk, bool sums = false) { return (size_t) 8 * mk_ls(nbk) + (sums ? (size_t) 32 * nbk : 0); }       // where a row's d start
__host__ __device__ __forceinline__ size_t mk_row_bytes(int nbk, bool sums = false) { return (mk_xd_off(nbk, sums) + (size_t) 4 * nbk + 15) & ~(size_t) 15; }

// quantize_row_q8_K_ref of one block held by a wave, lane i with elements i, 64 + i, 128 + i, 192 + i of it (v[0..3]: how a LayerNorm row and a
// swept run of granules lie in a wave) -> the operand row `op` (block blk of nbk).  The scale comes from the FIRST element of largest magnitude, with
// its sign: a lane's lowest such element by strict comparison in index order, then the lowest index over the wave (k_quantize_q8_K's rule for
// this distribution of the elements).  All lanes take part.  SUMS: the block's bsums as well (mk_xd_off) - register k holds element 64 k + lane, so sum
// 4 k + (lane >> 4) is register k's quant added up over one 16-lane DPP row (integers: exact in any order; an all-zero block has zero quants and zero sums)
//
// R4 (Q4_K, wa_quant4.h): the row may be one that the reference quantises in a group of four, ggml_quantize_mat_q8_K_4x8 (wa_q8_K_row4) - `row4`, the
// same for the whole wave.  That rule takes the sign from ANY element equal to + max|x| (iscale = -127 / max|x| then, else + 127 / max|x|: a block that
// holds - m before + m gets the opposite d and quants of the row rule) and saturates the quants to [-128, 127]; d = 1 / iscale and the sums as above.
// Without R4 nothing of it is compiled.
template <bool SUMS = false, bool R4 = false>
__device__ __forceinline__ void mk_quant_block(const float (&v)[4], int lane, unsigned char * op, int nbk, int blk, bool row4 = false) {
    float amax = fabsf(v[0]); int at = lane;
#pragma unroll
    for (int k = 1; k < 4; ++k) if (fabsf(v[k]) > amax) { amax = fabsf(v[k]); at = 64 * k + lane; }
    const float wmax = wave_max(amax);
    int first = amax == wmax ? at : 256;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, WAVE));
    const int fk = first >> 6;
    float max = __shfl(fk == 0 ? v[0] : fk == 1 ? v[1] : fk == 2 ? v[2] : v[3], first & 63, WAVE);
    if constexpr (R4) {
        const bool pos = v[0] == wmax || v[1] == wmax || v[2] == wmax || v[3] == wmax;
        if (row4) max = __any(pos) ? wmax : -wmax;
    }
    const float iscale = wmax != 0.0f ? -127.f / max : 0.0f;
    const float dq = wmax != 0.0f ? 1.0f / iscale : 0.0f;
    unsigned char * run = op + (size_t) ((lane & 31) >> 2) * mk_ls(nbk) + (size_t) blk * 32 + (lane >> 5) * 4;      // element 64 k + i: group 2 k + (i >> 5), lane (i & 31) >> 2, byte i & 3
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int qi = wmax != 0.0f ? min(127, (int) rintf(iscale * v[k])) : 0;
        if constexpr (R4) qi = row4 && qi < -128 ? -128 : qi;
        const unsigned q = (unsigned) qi & 0xffu;
        const unsigned w = q | (dpp_u32<0x101>(q) << 8) | (dpp_u32<0x102>(q) << 16) | (dpp_u32<0x103>(q) << 24);      // row_shl:1..3
        if ((lane & 3) == 0) *(unsigned *) (run + 8 * k) = w;
        if constexpr (SUMS) {
            int s = qi;
            s += __builtin_amdgcn_update_dpp(0, s, 0x128, 0xf, 0xf, true);      // row_ror:8, 4, 2, 1: the row's sum in every lane of it
            s += __builtin_amdgcn_update_dpp(0, s, 0x124, 0xf, 0xf, true);
            s += __builtin_amdgcn_update_dpp(0, s, 0x122, 0xf, 0xf, true);
            s += __builtin_amdgcn_update_dpp(0, s, 0x121, 0xf, 0xf, true);
            if ((lane & 15) == 0) ((short *) (op + (size_t) 8 * mk_ls(nbk)))[16 * blk + 4 * k + (lane >> 4)] = (short) s;
        }
    }
    if (lane == 0) ((float *) (op + mk_xd_off(nbk, SUMS)))[blk] = dq;
}

// wa_load.h - launchers of the model loader's device unpack kernels (wa_load.hip): a run of whole rows of a tensor as the file holds them,
// in a device staging buffer, -> the arena arrays of those rows.  The layouts are the ones the host functions state - wa_q32_unpack_rows
// (wa_quant1.h), wa_qk_unpack_rows (wa_quantk.h), wa_conv_reorder_rows below - and the kernels are held to them bit for bit
// (tests/test_load_kernels_gpu.py).  No HIP include: `stream` is a hipStream_t handed over as a pointer, the return value a hipError_t as
// an int (0 = launched).  Every launcher enqueues and returns; none allocates or synchronises.  The destination pointers are those of the
// run's FIRST row.
#pragma once
#include <cstddef>
#include <cstdint>

// 32-value formats, ggml type 6 Q5_0 / 8 Q8_0 / 3 Q4_1 / 7 Q5_1: quants [row][8][nb][4], scales [row][nb], minimums [row][nb] (types 3 and 7; else null).
// 16-byte stores where nb % 4 == 0 and the arrays are 16-byte aligned, 4-byte stores otherwise.
int wa_launch_load_q32(void * stream, int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, float * qd, float * qm);
// K formats, type 10 Q2_K / 11 Q3_K / 13 Q5_K / 14 Q6_K: quants [row][8][nb][8][4], scale bytes [row][nb][16], d [row][nb], dmin [row][nb] (types 10 and 13; else null)
int wa_launch_load_qk(void * stream, int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, int8_t * qsc, float * qd, float * qm);
// conv weights, F16: `rows` output channels of file order [oc][ic][3] -> dst [oc][k * IC + ic] with row stride ld elements, and the
// same bytes unchanged -> copy [oc][ic][3]
int wa_launch_load_conv(void * stream, const uint16_t * src, size_t rows, int IC, int ld, uint16_t * dst, uint16_t * copy);

// the host statement of the conv re-order
inline void wa_conv_reorder_rows(const uint16_t * src, size_t rows, int IC, int ld, uint16_t * dst, uint16_t * copy) {
    for (size_t i = 0; i < rows * (size_t) IC * 3; ++i) copy[i] = src[i];
    for (size_t oc = 0; oc < rows; ++oc)
        for (int ic = 0; ic < IC; ++ic)
            for (int k = 0; k < 3; ++k) dst[oc * (size_t) ld + (size_t) k * IC + ic] = src[(oc * (size_t) IC + ic) * 3 + k];
}

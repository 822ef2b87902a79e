// rows_q4k_quant.hip - the Q8_K quantiser of the several-rows decode step's Q4_K form (wa_rows_q8k_dev.h: mk_quant_block<true, true>) in isolation, on
// dictated F32 rows with a rule flag per row, beside the host functions it restates: wa_q8_K_row (the row rule) and wa_q8_K_row4 (the four-row rule).
// tests/test_rows_q4k_quant_gpu.py holds quants, d and bsums of the two to each other byte for byte.
#include "wa_rows_q8k_dev.h"
#include "wa_quant4.h"
#include <vector>

// a wave per row: lane i holds elements i, 64 + i, 128 + i, 192 + i of a block, as a LayerNorm row or a swept run of granules lies in a wave
__global__ void k_rows_q4k_quant(const float * x, int nbk, const int * row4, unsigned char * op, size_t op_bytes) {
    const int lane = threadIdx.x, r = blockIdx.x;
    for (int b = 0; b < nbk; ++b) {
        const float * xb = x + ((size_t) r * nbk + b) * 256;
        const float v[4] = { xb[lane], xb[64 + lane], xb[128 + lane], xb[192 + lane] };
        mk_quant_block<true, true>(v, lane, op + (size_t) r * op_bytes, nbk, b, row4[r] != 0);
    }
}

// x [rows][256 nbk], row4 [rows] -> q [rows][256 nbk] in element order, d [rows][nbk], bsums [rows][16 nbk].  0, or the HIP error
extern "C" int rows_q4k_quant(int rows, int nbk, const float * x, const int * row4, int8_t * q, float * d, int16_t * bsums) {
    const size_t opb = mk_row_bytes(nbk, true), nx = (size_t) rows * nbk * 256;
    float * dx = nullptr; int * dr = nullptr; unsigned char * dop = nullptr;
    hipError_t e = hipMalloc((void **) &dx, nx * 4);
    if (e == hipSuccess) e = hipMalloc((void **) &dr, (size_t) rows * 4);
    if (e == hipSuccess) e = hipMalloc((void **) &dop, rows * opb);
    if (e == hipSuccess) e = hipMemcpy(dx, x, nx * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dr, row4, (size_t) rows * 4, hipMemcpyHostToDevice);
    std::vector<unsigned char> op(rows * opb);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rows_q4k_quant, dim3(rows), dim3(64), 0, 0, dx, nbk, dr, dop, opb);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(op.data(), dop, rows * opb, hipMemcpyDeviceToHost);
    (void) hipFree(dx); (void) hipFree(dr); (void) hipFree(dop);
    if (e != hipSuccess) return (int) e;
    for (int r = 0; r < rows; ++r) {
        const unsigned char * o = op.data() + r * opb;
        for (int b = 0; b < nbk; ++b) {
            for (int el = 0; el < 256; ++el)      // element el: group el / 32, lane (el % 32) / 4, byte el % 4
                q[((size_t) r * nbk + b) * 256 + el] = (int8_t) o[(size_t) ((el & 31) >> 2) * mk_ls(nbk) + 32 * b + 4 * (el >> 5) + (el & 3)];
            memcpy(bsums + ((size_t) r * nbk + b) * 16, o + (size_t) 8 * mk_ls(nbk) + 32 * b, 32);
            memcpy(d + (size_t) r * nbk + b, o + mk_xd_off(nbk, true) + 4 * b, 4);
        }
    }
    return 0;
}

extern "C" void rows_q4k_quant_host(int rows, int nbk, const float * x, const int * row4, int8_t * q, float * d, int16_t * bsums) {
    for (int r = 0; r < rows; ++r) {
        const size_t o = (size_t) r * nbk;
        if (row4[r]) wa_q8_K_row4(x + o * 256, nbk, q + o * 256, d + o, bsums + o * 16);
        else         wa_q8_K_row(x + o * 256, nbk, q + o * 256, d + o, bsums + o * 16);
    }
}

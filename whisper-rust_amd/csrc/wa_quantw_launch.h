// wa_quantw_launch.h - launcher of the weight-quantising kernels (wa_quantw.hip): a run of F32 or F16 values in device memory -> standard
// ggml blocks in the file's byte layout, the bytes wa_quantw_rows (wa_quantw.h) gives.  No HIP include: `stream` is a hipStream_t handed over
// as a pointer, the return value a hipError_t as an int (0 = launched).  The launcher enqueues and returns; it neither allocates nor
// synchronises.
#pragma once
#include <cstddef>
#include <cstdint>

// type: ggml type 2 Q4_0 / 3 Q4_1 / 6 Q5_0 / 7 Q5_1 / 8 Q8_0 / 12 Q4_K / 13 Q5_K / 14 Q6_K.  src: nblocks * (32 or 256) values, 16-byte aligned;
// dst: nblocks (at most 2^31 - 1: what a grid holds) blocks, 4-byte aligned (16-byte stores where it is 16-byte aligned).  *flag (device memory, cleared by the caller) is set
// to 1 when a source value is not finite; the blocks of such a run mean nothing.
int wa_launch_quantw(void * stream, int type, const void * src, int src_is_f16, size_t nblocks, uint8_t * dst, uint32_t * flag);

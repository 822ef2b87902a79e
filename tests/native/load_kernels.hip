// load_kernels.hip - TEST INFRASTRUCTURE ONLY: a C entry point per launcher of wa_load.hip (the model loader's unpack kernels), for
// tests/test_load_kernels_gpu.py.  Linked against the product's own whisper-rust_amd/build/wa_load.o (whisper-rust_amd/Makefile, target
// `load_harness`), so the kernels under test are the ones libwhisper.so ships.  Every launch goes to the null stream; ltest_sync() waits
// for it and reports the first HIP error.
#include "wa_load.h"

#include <hip/hip_runtime.h>

#define LT_API extern "C" __attribute__((visibility("default")))

LT_API void * ltest_alloc(size_t bytes) {
    void * p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
LT_API int ltest_free(void * p) { return (int) hipFree(p); }
LT_API int ltest_h2d(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
LT_API int ltest_d2h(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
LT_API int ltest_sync() {
    const hipError_t e = hipDeviceSynchronize();
    const hipError_t l = hipGetLastError();
    return (int) (e != hipSuccess ? e : l);
}

LT_API int ltest_load_q32(int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, float * qd, float * qm) {
    return wa_launch_load_q32(nullptr, type, src, rows, nb, qs, qd, qm);
}
LT_API int ltest_load_qk(int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, int8_t * qsc, float * qd, float * qm) {
    return wa_launch_load_qk(nullptr, type, src, rows, nb, qs, qsc, qd, qm);
}
LT_API int ltest_load_conv(const uint16_t * src, size_t rows, int IC, int ld, uint16_t * dst, uint16_t * copy) {
    return wa_launch_load_conv(nullptr, src, rows, IC, ld, dst, copy);
}

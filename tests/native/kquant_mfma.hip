// kquant_mfma.hip - TEST INFRASTRUCTURE ONLY: the K-format product launcher of wa_quantk_mfma.hip with the kernel named (route 0: the launcher's own
// rule, 1: k_kgemm_exact / k_kgemv_exact, 3: the matrix-core kernel k_kgemm_mfma wherever it applies), and which kernel a route takes, for
// tests/test_kquant_mfma_gpu.py.  Linked against the product's own build/wa_quantk_mfma.o, wa_quantk.o and wa_quantk_q2.o (whisper-rust_amd/Makefile,
// target `kquant_harness`), so the kernels under test are the ones libwhisper.so ships.  Every launch goes to the null stream; kmtest_sync() waits
// for it and reports the first HIP error.
#include "wa_kernels.h"

#define KM_API extern "C" __attribute__((visibility("default")))

KM_API void * kmtest_alloc(size_t bytes) {
    void * p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
KM_API int kmtest_free(void * p) { return (int) hipFree(p); }
KM_API int kmtest_h2d(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
KM_API int kmtest_d2h(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
KM_API int kmtest_sync() {
    const hipError_t e = hipDeviceSynchronize();
    const hipError_t l = hipGetLastError();
    return (int) (e != hipSuccess ? e : l);
}

// The epilogue fields a test sets, as a flat C struct (the layout of tests/native/kquant_kernels.hip: ktest_epi).
struct kmtest_epi {
    const float * bias; const float * scale;
    void * out; int ldo;
    void * out2; int ldo2;
    void * out3; int ldo3;
    const float * resid; int ldr;
    const wa_f16 * gelu;
    int split0, split1, row_off, aux0, aux1;
};

KM_API void kmtest_kgemm(int route, int mode, int wtype, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq, const int8_t * wsc,
                         const float * wd, const float * wdm, int N, int K, const kmtest_epi * k) {
    wa_epi e;
    e.bias = k->bias; e.scale = k->scale;
    e.out = k->out; e.ldo = k->ldo; e.out2 = k->out2; e.ldo2 = k->ldo2; e.out3 = k->out3; e.ldo3 = k->ldo3;
    e.resid = k->resid; e.ldr = k->ldr; e.gelu = k->gelu;
    e.split0 = k->split0; e.split1 = k->split1; e.row_off = k->row_off; e.aux0 = k->aux0; e.aux1 = k->aux1;
    wa_launch_kgemm_route(nullptr, (wa_epi_mode) mode, wtype, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e, route);
}

// the kernel a route takes (1 k_kgemm_exact / k_kgemv_exact, 3 k_kgemm_mfma); launches nothing
KM_API int kmtest_kernel(int route, int mode, int wtype, int M, int N, int K, int has_rowp) {
    static const wa_rowptr none = {};
    wa_epi e;
    if (has_rowp) e.rowp = &none;          // (only looked at, never read through)
    return wa_kgemm_kernel((wa_epi_mode) mode, wtype, M, N, K, e, route);
}

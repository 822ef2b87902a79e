// kquant_kernels.hip - TEST INFRASTRUCTURE ONLY: a C entry point per launcher of wa_quantk.hip (the Q8_K quantiser, the Q5_K / Q6_K
// products with every epilogue, the token embedding), for tests/test_kquant_kernels_gpu.py.  Linked against the product's own
// whisper-rust_amd/build/wa_quantk.o (whisper-rust_amd/Makefile, target `kquant_harness`), so the kernels under test are the ones
// libwhisper.so ships.  Every launch goes to the null stream; ktest_sync() waits for it and reports the first HIP error.
#include "wa_kernels.h"

#define KT_API extern "C" __attribute__((visibility("default")))

KT_API void * ktest_alloc(size_t bytes) {
    void * p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
KT_API int ktest_free(void * p) { return (int) hipFree(p); }
KT_API int ktest_h2d(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
KT_API int ktest_d2h(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
KT_API int ktest_sync() {
    const hipError_t e = hipDeviceSynchronize();
    const hipError_t l = hipGetLastError();
    return (int) (e != hipSuccess ? e : l);
}

KT_API void ktest_quantize_q8_K(const float * x, int ldx, int rows, int K, int8_t * qs, float * qd, int16_t * qbs) {
    wa_launch_quantize_q8_K(nullptr, x, ldx, rows, K, qs, qd, qbs);
}

// The epilogue fields a test sets, as a flat C struct (the layout of tests/native/quant_kernels.hip: qtest_epi).
struct ktest_epi {
    const float * bias; const float * scale;
    void * out; int ldo;
    void * out2; int ldo2;
    void * out3; int ldo3;
    const float * resid; int ldr;
    const wa_f16 * gelu;
    int split0, split1, row_off, aux0, aux1;
};

KT_API void ktest_kgemm_exact(int mode, int wtype, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq, const int8_t * wsc,
                              const float * wd, const float * wdm, int N, int K, const ktest_epi * k) {
    wa_epi e;
    e.bias = k->bias; e.scale = k->scale;
    e.out = k->out; e.ldo = k->ldo; e.out2 = k->out2; e.ldo2 = k->ldo2; e.out3 = k->out3; e.ldo3 = k->ldo3;
    e.resid = k->resid; e.ldr = k->ldr; e.gelu = k->gelu;
    e.split0 = k->split0; e.split1 = k->split1; e.row_off = k->row_off; e.aux0 = k->aux0; e.aux1 = k->aux1;
    wa_launch_kgemm_exact(nullptr, (wa_epi_mode) mode, wtype, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e);
}

KT_API void ktest_dec_embed_k(int wtype, const int32_t * tok, const int32_t * pos, int n_tokens, int d, const int8_t * wq, const int8_t * wsc, const float * wd,
                              const float * wdm, const float * pe, float * x) {
    wa_launch_dec_embed_k(nullptr, wtype, tok, pos, n_tokens, d, wq, wsc, wd, wdm, pe, x);
}

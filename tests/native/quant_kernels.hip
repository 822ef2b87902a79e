// quant_kernels.hip - TEST INFRASTRUCTURE ONLY: a C entry point per launcher of wa_quant.hip (the Q8_0 / Q8_1 quantiser, the quantised
// products with every epilogue, the fused GELU product, the quantised token embedding), for tests/test_quant_kernels_gpu.py.  Linked
// against the product's own whisper-rust_amd/build/wa_quant.o (oracle/Makefile, target `harness`), so the kernels under test are the
// ones libwhisper.so ships.  Every launch goes to the null stream; qtest_sync() waits for it and reports the first HIP error.
#include "wa_kernels.h"

#define QT_API extern "C" __attribute__((visibility("default")))

QT_API void * qtest_alloc(size_t bytes) {
    void * p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
QT_API int qtest_free(void * p) { return (int) hipFree(p); }
QT_API int qtest_h2d(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
QT_API int qtest_d2h(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
QT_API int qtest_sync() {
    const hipError_t e = hipDeviceSynchronize();
    const hipError_t l = hipGetLastError();
    return (int) (e != hipSuccess ? e : l);
}

QT_API void qtest_quantize_q8_0(const float * x, int ldx, int rows, int K, int8_t * qs, float * qd, float * qsum) {
    wa_launch_quantize_q8_0(nullptr, x, ldx, rows, K, qs, qd, qsum);
}

// The epilogue fields a test sets, as a flat C struct (wa_epi has default member initialisers; Python never mirrors it).
// dyn, the batch strides and rowp stay at their defaults.
struct qtest_epi {
    const float * bias; const float * scale;
    void * out; int ldo;
    void * out2; int ldo2;
    void * out3; int ldo3;
    const float * resid; int ldr;
    const wa_f16 * gelu;
    int split0, split1, row_off, aux0, aux1;
};

// xs / wm null: the Q5_0 / Q8_0 product; both set: Q4_1 / Q5_1
QT_API void qtest_qgemm_exact(int mode, const int8_t * xq, const float * xd, int M, const int8_t * wq, const float * wd, int N, int K, const qtest_epi * k,
                              const float * xs, const float * wm) {
    wa_epi e;
    e.bias = k->bias; e.scale = k->scale;
    e.out = k->out; e.ldo = k->ldo; e.out2 = k->out2; e.ldo2 = k->ldo2; e.out3 = k->out3; e.ldo3 = k->ldo3;
    e.resid = k->resid; e.ldr = k->ldr; e.gelu = k->gelu;
    e.split0 = k->split0; e.split1 = k->split1; e.row_off = k->row_off; e.aux0 = k->aux0; e.aux1 = k->aux1;
    wa_launch_qgemm_exact(nullptr, (wa_epi_mode) mode, xq, xd, M, wq, wd, N, K, e, xs, wm);
}

QT_API void qtest_qgemv_gelu_q8(const int8_t * xq, const float * xd, const int8_t * wq, const float * wd, int N, int K, const float * bias, const wa_f16 * gelu,
                                int8_t * oq, float * oqd, const float * xs, const float * wm, float * oqs) {
    wa_launch_qgemv_gelu_q8(nullptr, xq, xd, wq, wd, N, K, bias, gelu, oq, oqd, xs, wm, oqs);
}

QT_API void qtest_dec_embed_q(const int32_t * tok, const int32_t * pos, int n_tokens, int d, const int8_t * wq, const float * wd, const float * pe, float * x,
                              const float * wm) {
    wa_launch_dec_embed_q(nullptr, tok, pos, n_tokens, d, wq, wd, pe, x, wm);
}

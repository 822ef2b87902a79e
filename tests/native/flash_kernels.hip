// flash_kernels.hip - TEST INFRASTRUCTURE ONLY: a C entry point per tolerance-path launcher of wa_kernels.hip
// (flash_attn = true), for tests/test_flash_kernels_gpu.py.  Linked against the product's own whisper-rust_amd/build/wa_kernels.o
// (oracle/Makefile, target `harness`), so the kernels under test are the ones libwhisper.so ships.  Every launch goes to the null
// stream; ktest_sync() waits for it and reports the first HIP error.
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

// The epilogue fields a test sets, as a flat C struct (wa_epi has default member initialisers; Python never mirrors it).
// dyn, the batch strides and rowp stay at their defaults: those are the decode step's, not the flash path's.
struct ktest_epi {
    const float * bias; const float * scale;
    void * out; int ldo;
    void * out2; int ldo2;
    void * out3; int ldo3;
    const float * resid; int ldr;
    float * dbg;
    const wa_f16 * gelu;
    int split0, split1, row_off, aux0, aux1;
};

KT_API void ktest_gemm(int mode, const wa_f16 * A, int lda, const wa_f16 * W, int ldw, int M, int N, int K, const ktest_epi * k) {
    wa_epi e;
    e.bias = k->bias; e.scale = k->scale;
    e.out = k->out; e.ldo = k->ldo; e.out2 = k->out2; e.ldo2 = k->ldo2; e.out3 = k->out3; e.ldo3 = k->ldo3;
    e.resid = k->resid; e.ldr = k->ldr; e.dbg = k->dbg; e.gelu = k->gelu;
    e.split0 = k->split0; e.split1 = k->split1; e.row_off = k->row_off; e.aux0 = k->aux0; e.aux1 = k->aux1;
    wa_launch_gemm(nullptr, (wa_epi_mode) mode, A, lda, W, ldw, M, N, K, e);
}

KT_API void ktest_layernorm(const float * x, int ldx, int rows, int d, const float * w, const float * b, float eps, wa_f16 * out16, int ld16,
                            float * out32, int ld32) {
    wa_launch_layernorm(nullptr, x, ldx, rows, d, w, b, eps, out16, ld16, out32, ld32);
}

KT_API void ktest_enc_attn(const wa_f16 * qk, int ldqk, const wa_f16 * vt, int ldvt, int T, int d, int n_head, float scale, wa_f16 * out, int ldo) {
    wa_launch_enc_attn(nullptr, qk, ldqk, vt, ldvt, T, d, n_head, scale, out, ldo);
}

// exact_kernels.hip - TEST INFRASTRUCTURE ONLY: a C entry point per reference-order launcher of wa_exact.hip that takes a certified
// F64 sum (LayerNorm statistics, soft-max denominators), for tests/test_exact_sums_gpu.py.  Linked against the product's own
// whisper-rust_amd/build/wa_exact.o (oracle/Makefile, target `harness`), so the kernels under test are the ones libwhisper.so ships.
// Every launch goes to the null stream; xtest_sync() waits for it and reports the first HIP error.
#include "wa_kernels.h"

#define XT_API extern "C" __attribute__((visibility("default")))

XT_API void * xtest_alloc(size_t bytes) {
    void * p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
XT_API int xtest_free(void * p) { return (int) hipFree(p); }
XT_API int xtest_h2d(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
XT_API int xtest_d2h(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
XT_API int xtest_sync() {
    const hipError_t e = hipDeviceSynchronize();
    const hipError_t l = hipGetLastError();
    return (int) (e != hipSuccess ? e : l);
}

XT_API void xtest_layernorm_exact(const float * x, int ldx, int rows, int d, const float * w, const float * b, float eps, wa_f16 * out16, int ld16,
                                  float * out32, int ld32, int8_t * qs, float * qd, float * qsum) {
    wa_launch_layernorm_exact(nullptr, x, ldx, rows, d, w, b, eps, out16, ld16, out32, ld32, qs, qd, qsum);
}

// out f32 [M][ldo] = LayerNorm(x) (rounded to F16) . W^T, mode WA_EPI_F32 without a bias
XT_API void xtest_ln_gemv_exact_f32(const float * x, int ldx, const float * ln_w, const float * ln_b, float eps, const wa_f16 * W, int ldw, int M, int N, int K,
                                    float * out, int ldo) {
    wa_epi e;
    e.out = out; e.ldo = ldo;
    wa_launch_ln_gemv_exact(nullptr, WA_EPI_F32, x, ldx, nullptr, ln_w, ln_b, eps, W, ldw, M, N, K, e);
}

XT_API void xtest_ln_q8_row(const float * x, int K, const float * w, const float * b, float eps, int8_t * qs, float * qd, float * qsum) {
    wa_launch_ln_q8_row(nullptr, x, K, w, b, eps, qs, qd, qsum);
}

// no dyn, no quantised rows, no per-row states: the forms the launch sequence of an F16 model uses
XT_API void xtest_attn_exact(const wa_f16 * q, int ldq, const wa_f16 * kbase, size_t k_head_stride, int k_row_stride, const wa_f16 * vbase, size_t v_head_stride,
                             int v_row_stride, int n_head, int n_tokens, int n_kv, const int8_t * mask, float scale, float * partial, wa_f16 * p_left,
                             wa_f16 * out, int ldo, float * qk_out) {
    wa_launch_attn_exact(nullptr, q, ldq, kbase, k_head_stride, k_row_stride, vbase, v_head_stride, v_row_stride, n_head, n_tokens, n_kv, mask, scale, partial,
                         p_left, out, ldo, qk_out);
}

XT_API void xtest_attn_exact_mfma(const wa_f16 * qk, int ldqk, const wa_f16 * vt, int ldvt, int T, int d, int n_head, float scale, wa_f16 * p, wa_f16 * p_left,
                                  int kvp, wa_f16 * out, int ldo) {
    wa_launch_attn_exact_mfma(nullptr, qk, ldqk, vt, ldvt, T, d, n_head, scale, p, p_left, kvp, out, ldo);
}

// fewrows_kernels.hip - TEST INFRASTRUCTURE ONLY: the quantised products with the kernel named (wa_launch_qgemm_exact_route: the launcher's rule, the
// general kernel k_qgemm_exact, the few-rows kernel k_qgemv_rows) and with rows of different states (wa_epi::rowp), for
// tests/test_quant_fewrows_gpu.py.  Linked against the product's own build/wa_quant.o, wa_quantk.o and wa_quantk_q2.o (whisper-rust_amd/Makefile,
// target kquant_harness), so the kernels under test are the ones libwhisper.so ships.  Every launch goes to the null stream; frtest_sync() waits
// for it and reports the first HIP error.
#include "wa_kernels.h"

#define FR_API extern "C" __attribute__((visibility("default")))

FR_API void * frtest_alloc(size_t bytes) {
    void * p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
FR_API int frtest_free(void * p) { return (int) hipFree(p); }
FR_API int frtest_h2d(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
FR_API int frtest_d2h(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
FR_API int frtest_sync() {
    const hipError_t e = hipDeviceSynchronize();
    const hipError_t l = hipGetLastError();
    return (int) (e != hipSuccess ? e : l);
}
FR_API int frtest_rowptr_bytes() { return (int) sizeof(wa_rowptr); }

// The epilogue fields a test sets (wa_epi has default member initialisers; Python never mirrors it).  rowp: device array of M wa_rowptr
// { kv_k, kv_v, cross_k, cross_v, n_kv, kv_head } or null.
struct frtest_epi {
    const float * bias; const float * scale;
    void * out; int ldo;
    void * out2; int ldo2;
    void * out3; int ldo3;
    const float * resid; int ldr;
    const wa_f16 * gelu;
    int split0, split1, row_off, aux0, aux1;
    const void * rowp; long long rowp_off;
};
static wa_epi to_epi(const frtest_epi * k) {
    wa_epi e;
    e.bias = k->bias; e.scale = k->scale;
    e.out = k->out; e.ldo = k->ldo; e.out2 = k->out2; e.ldo2 = k->ldo2; e.out3 = k->out3; e.ldo3 = k->ldo3;
    e.resid = k->resid; e.ldr = k->ldr; e.gelu = k->gelu;
    e.split0 = k->split0; e.split1 = k->split1; e.row_off = k->row_off; e.aux0 = k->aux0; e.aux1 = k->aux1;
    e.rowp = (const wa_rowptr *) k->rowp; e.rowp_off = k->rowp_off;
    return e;
}

// route 0: the launcher's rule, 1: k_qgemm_exact, 2: k_qgemv_rows.  xs / wm null: the Q5_0 / Q8_0 product; both set: Q4_1 / Q5_1
FR_API void frtest_qgemm(int route, int mode, const int8_t * xq, const float * xd, int M, const int8_t * wq, const float * wd, int N, int K, const frtest_epi * k,
                         const float * xs, const float * wm) {
    wa_launch_qgemm_exact_route(nullptr, (wa_epi_mode) mode, xq, xd, M, wq, wd, N, K, to_epi(k), xs, wm, route);
}
FR_API void frtest_kgemm(int mode, int wtype, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq, const int8_t * wsc,
                         const float * wd, const float * wdm, int N, int K, const frtest_epi * k) {
    wa_launch_kgemm_exact(nullptr, (wa_epi_mode) mode, wtype, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, to_epi(k));
}

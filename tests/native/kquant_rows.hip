// kquant_rows.hip - TEST INFRASTRUCTURE ONLY: the K-format product launcher of wa_quantk_rows.hip with the kernel named (route 0: the launchers' own
// rules, 1: never the few-rows kernel, 2: k_kgemv_rows wherever it exists), and which kernel a route takes, for tests/test_kquant_fewrows_gpu.py.
// Linked against the product's own build/wa_quantk_rows.o, wa_quantk_mfma.o, wa_quantk.o and wa_quantk_q2.o (whisper-rust_amd/Makefile, target
// `kquant_harness`), so the kernels under test are the ones libwhisper.so ships.  Every launch goes to the null stream; krtest_sync() waits for it
// and reports the first HIP error.
#include "wa_kernels.h"

#define KR_API extern "C" __attribute__((visibility("default")))

KR_API void * krtest_alloc(size_t bytes) {
    void * p = nullptr;
    return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
KR_API int krtest_free(void * p) { return (int) hipFree(p); }
KR_API int krtest_h2d(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice); }
KR_API int krtest_d2h(void * dst, const void * src, size_t bytes) { return (int) hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost); }
KR_API int krtest_sync() {
    const hipError_t e = hipDeviceSynchronize();
    const hipError_t l = hipGetLastError();
    return (int) (e != hipSuccess ? e : l);
}
KR_API int krtest_rowptr_bytes() { return (int) sizeof(wa_rowptr); }

// The epilogue fields a test sets, as a flat C struct (the layout of tests/native/fewrows_kernels.hip: frtest_epi).  rowp: device array of M wa_rowptr
// { kv_k, kv_v, cross_k, cross_v, n_kv, kv_head } or null.
struct krtest_epi {
    const float * bias; const float * scale;
    void * out; int ldo;
    void * out2; int ldo2;
    void * out3; int ldo3;
    const float * resid; int ldr;
    const wa_f16 * gelu;
    int split0, split1, row_off, aux0, aux1;
    const void * rowp; long long rowp_off;
};

KR_API void krtest_kgemm(int route, int mode, int wtype, const int8_t * xq, const float * xd, const int16_t * xbs, int M, const int8_t * wq, const int8_t * wsc,
                         const float * wd, const float * wdm, int N, int K, const krtest_epi * k) {
    wa_epi e;
    e.bias = k->bias; e.scale = k->scale;
    e.out = k->out; e.ldo = k->ldo; e.out2 = k->out2; e.ldo2 = k->ldo2; e.out3 = k->out3; e.ldo3 = k->ldo3;
    e.resid = k->resid; e.ldr = k->ldr; e.gelu = k->gelu;
    e.split0 = k->split0; e.split1 = k->split1; e.row_off = k->row_off; e.aux0 = k->aux0; e.aux1 = k->aux1;
    e.rowp = (const wa_rowptr *) k->rowp; e.rowp_off = k->rowp_off;
    wa_launch_kgemm_few_route(nullptr, (wa_epi_mode) mode, wtype, xq, xd, xbs, M, wq, wsc, wd, wdm, N, K, e, route);
}

// HOST code: the Q2_K product as wa_quantk.hip states it, in the kernel layout, with the minimum term of a block before its product term
// (min_after == 0: the reference's order; the test holds this to libkquant_ref.so) or after it (min_after == 1: the wrong order, which the test
// shows to give other bits).  out [M][N].
KR_API void krtest_q2_host(int M, int N, int K, const int8_t * wq, const uint8_t * wsc, const float * wd, const float * wdm, const int8_t * xq, const float * xd,
                           const int16_t * xbs, float * out, int min_after) {
    const size_t nb = (size_t) K / 256;
    for (size_t m = 0; m < (size_t) M; ++m)
        for (size_t n = 0; n < (size_t) N; ++n) {
            float acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            for (size_t b = 0; b < nb; ++b) {
                const uint8_t * sc = wsc + (n * nb + b) * 16;
                const int16_t * bs = xbs + (m * nb + b) * 16;
                const float dx = xd[m * nb + b], dd = dx * wd[n * nb + b], dn = -dx * wdm[n * nb + b];
                for (size_t l = 0; l < 8; ++l) {
                    const int8_t * w = wq + ((n * 8 + l) * nb + b) * 32, * x = xq + ((m * 8 + l) * nb + b) * 32;
                    int sumi = 0;
                    for (int g = 0; g < 8; ++g) {
                        int s4 = 0;
                        for (int i = 0; i < 4; ++i) s4 += (int) w[4 * g + i] * (int) x[4 * g + i];
                        sumi += (int) (sc[8 * (l >> 2) + g] & 15) * s4;
                    }
                    const int mins = (int) (sc[l] >> 4) * (int) bs[2 * l] + (int) (sc[8 + l] >> 4) * (int) bs[2 * l + 1];
                    if (!min_after) acc[l] = fmaf(dn, (float) mins, acc[l]);
                    acc[l] = fmaf(dd, (float) sumi, acc[l]);
                    if (min_after) acc[l] = fmaf(dn, (float) mins, acc[l]);
                }
            }
            out[m * N + n] = ((acc[0] + acc[4]) + (acc[2] + acc[6])) + ((acc[1] + acc[5]) + (acc[3] + acc[7]));
        }
}

// the kernel a route takes (1 k_kgemm_exact / k_kgemv_exact, 2 k_kgemv_rows, 3 k_kgemm_mfma); launches nothing
KR_API int krtest_kernel(int route, int mode, int wtype, int M, int N, int K, int has_rowp) {
    static const wa_rowptr none = {};
    wa_epi e;
    if (has_rowp) e.rowp = &none;          // (only looked at, never read through)
    return wa_kgemm_few_kernel((wa_epi_mode) mode, wtype, M, N, K, e, route);
}

// qmfma_route.hip - TEST INFRASTRUCTURE ONLY: which kernel wa_launch_qgemm_exact_route takes for a product and a route (wa_qgemm_exact_kernel:
// 1 k_qgemm_exact / k_qgemv_exact, 2 k_qgemv_rows, 3 k_qgemm_mfma), for tests/test_quant_mfma_gpu.py - the kernels give the same bits, so the
// results cannot tell.  Linked against the product's own build/wa_quant.o (whisper-rust_amd/Makefile, target kquant_harness).  Launches nothing.
#include "wa_kernels.h"

extern "C" __attribute__((visibility("default"))) int qmtest_kernel(int route, int mode, int M, int N, int K, int rowp_set) {
    static const wa_rowptr none = {};
    wa_epi e;
    if (rowp_set) e.rowp = &none;          // (only looked at, never read through)
    return wa_qgemm_exact_kernel((wa_epi_mode) mode, M, N, K, e, route);
}

// align_kernels.hip - tests/test_align_kernels_gpu.py: k_align_score alone, through the launcher of the product's own wa_align_k.o.
//
// align_kernels_run copies the caller's rows [n_rows][ld] into a device buffer whose first row begins `off` floats (0..3) behind a 16-byte
// boundary, so that the test decides which rows the kernel reads through its 16-byte path and which head and tail it leaves to scalar
// loads; the floats in front of the first row and behind the last element hold NaN (a read past either end would show in the scores).
#include "wa_align.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <limits>
#include <vector>

#define CK(x) do { if ((x) != hipSuccess) { rc = -1; goto done; } } while (0)

extern "C" __attribute__((visibility("default")))
int align_kernels_run(const float * logits, long long ld, int n_rows, int n_vocab, const int32_t * target, int off, struct whisper_amd_align_score * out) {
    if (!logits || !target || !out || n_rows <= 0 || n_vocab <= 0 || ld < n_vocab || off < 0 || off > 3) return -2;
    const size_t n_used = (size_t) (n_rows - 1) * ld + n_vocab, n_all = 4 + n_used + 4;
    std::vector<float> host(n_all, std::numeric_limits<float>::quiet_NaN());
    for (int r = 0; r < n_rows; ++r) memcpy(host.data() + off + (size_t) r * ld, logits + (size_t) r * ld, (size_t) n_vocab * sizeof(float));
    float * d_x = nullptr; int32_t * d_t = nullptr; struct whisper_amd_align_score * d_o = nullptr;
    int rc = 0;
    CK(hipMalloc((void **) &d_x, n_all * sizeof(float)));
    CK(hipMalloc((void **) &d_t, (size_t) n_rows * sizeof(int32_t)));
    CK(hipMalloc((void **) &d_o, (size_t) n_rows * sizeof(*d_o)));
    CK(hipMemcpy(d_x, host.data(), n_all * sizeof(float), hipMemcpyHostToDevice));
    CK(hipMemcpy(d_t, target, (size_t) n_rows * sizeof(int32_t), hipMemcpyHostToDevice));
    CK(hipMemset(d_o, 0xff, (size_t) n_rows * sizeof(*d_o)));
    if (!wa_align_score_launch(nullptr, d_x + off, ld, n_rows, n_vocab, d_t, d_o)) { rc = -3; goto done; }
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(out, d_o, (size_t) n_rows * sizeof(*d_o), hipMemcpyDeviceToHost));
done:
    if (d_x) (void) hipFree(d_x);
    if (d_t) (void) hipFree(d_t);
    if (d_o) (void) hipFree(d_o);
    return rc;
}

// the host restatement behind the same library, for the comparison of best_id and rank
extern "C" __attribute__((visibility("default")))
void align_kernels_host(const float * logits, long long ld, int n_rows, int n_vocab, const int32_t * target, struct whisper_amd_align_score * out) {
    wa_align_score_host(logits, ld, n_rows, n_vocab, target, out);
}

// align_math.cpp - tests/test_align_math.py: the host restatement of the alignment scores (whisper-rust_amd/csrc/wa_align.h) behind one C entry
// point, compiled alone by g++ (-ffp-contract=off, as the product's host code): no HIP, no device.
#include "wa_align.h"

extern "C" void align_math_score(const float * logits, long long ld, int n_rows, int n_vocab, const int32_t * target, struct whisper_amd_align_score * out) {
    wa_align_score_host(logits, ld, n_rows, n_vocab, target, out);
}

extern "C" int align_math_sizes(int which) {
    return which == 0 ? (int) sizeof(struct whisper_amd_align_score) : (int) sizeof(struct whisper_amd_align_token);
}

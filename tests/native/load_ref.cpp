// load_ref.cpp - TEST INFRASTRUCTURE ONLY: the host functions that define what the model loader writes into the weight arena - the ones
// its host path runs (whisper-rust_amd/csrc/wa_quant1.h, wa_quantk.h, wa_load.h) - behind C entry points, as the yardstick of
// tests/test_load_kernels_gpu.py.  Nothing is restated here.  g++ alone.
#include "wa_load.h"
#include "wa_quant1.h"
#include "wa_quantk.h"

#define LR_API extern "C" __attribute__((visibility("default")))

LR_API void lref_q32(int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, float * qd, float * qm) {
    wa_q32_unpack_rows(type, src, rows, nb, qs, qd, qm);
}
LR_API void lref_qk(int type, const uint8_t * src, size_t rows, size_t nb, int8_t * qs, int8_t * qsc, float * qd, float * qm) {
    wa_qk_unpack_rows(type, src, rows, nb, qs, qsc, qd, qm);
}
LR_API void lref_conv(const uint16_t * src, size_t rows, int IC, int ld, uint16_t * dst, uint16_t * copy) {
    wa_conv_reorder_rows(src, rows, IC, ld, dst, copy);
}
// one block, element order: what the dictated blocks of the tests are read back with
LR_API void lref_q32_block(int type, const uint8_t * blk, int8_t q[32], float * d, float * m) {
    *m = 0.0f;
    if (wa_q1_block_bytes(type)) wa_q1_unpack(type, blk, q, *d, *m); else wa_q0_unpack(type, blk, q, *d);
}
LR_API void lref_qk_block(int type, const uint8_t * blk, int8_t q[256], int8_t sc[16], float * d, float * dmin) { wa_qk_unpack(type, blk, q, sc, *d, *dmin); }

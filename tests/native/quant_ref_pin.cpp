// Variant 0 of tests/native/quant_ref.cpp (the expected values of tests/test_quant_kernels_gpu.py) against the reference library's own
// exported functions, bit for bit: the Q5_0 / Q8_0 product against ggml_vec_dot_q5_0_q8_0 / ggml_vec_dot_q8_0_q8_0 and the quantiser
// against quantize_row_q8_0.  (The Q4_1 / Q5_1 side of the same file is wa_quant1.h itself, which quant1_math.cpp holds.)
// Rows as in quant1_math.cpp - (a) the reference's own quantiser on Gaussian weights, (b) raw blocks, (c) the rounding points of the
// activation row, (d) weights far from zero - at K = 32 .. 3072, plus Q8_0 weight bytes of -128, which a raw file may hold.
// argv[1] = path of the reference library.  Prints "quant_ref: N mismatches" (N = 0 is the pass).
#include "quant_ref.cpp"

#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef void (*quant_fn)(const float *, void *, int64_t);
typedef void (*dot_fn)(int, float *, size_t, const void *, size_t, const void *, size_t, int);

static quant_fn q8_0, q5_0_ref, q8_0_ref;
static dot_fn dot5_0, dot8_0;
static long n_bad = 0, n_checked = 0;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
static void bad(const char * what, int type, int K, long i, float got, float want) {
    if (n_bad < 20) printf("MISMATCH %s type %d K %d at %ld: got %a (%08x) want %a (%08x)\n", what, type, K, i, got, bits(got), want, bits(want));
    n_bad += 1;
}

// block_q5_0 { f16 d; u8 qh[4]; u8 qs[16]; } 22 bytes, block_q8_0 { f16 d; i8 qs[32]; } 34 bytes
static size_t block_bytes(int type) { return type == 6 ? 22 : 34; }

// one block on file -> its 32 signed quants and scale; Q5_0: (nibble | bit << 4) - 16
static void unpack(int type, const uint8_t * blk, int8_t q[32], float & d) {
    uint16_t dh; memcpy(&dh, blk, 2);
    d = wa_q1_h2f(dh);
    if (type == 8) { memcpy(q, blk + 2, 32); return; }
    uint32_t qh; memcpy(&qh, blk + 2, 4);
    const uint8_t * qs = blk + 6;
    for (int j = 0; j < 16; ++j) {
        q[j]      = (int8_t) (((qs[j] & 0x0f) | (((qh >> j) & 1u) << 4)) - 16);
        q[j + 16] = (int8_t) (((qs[j] >> 4)   | (((qh >> (j + 16)) & 1u) << 4)) - 16);
    }
}

// weight rows given as raw blocks (type 6: Q5_0, type 8: Q8_0) x one activation row
static void check(int type, int K, int n_rows, const std::vector<uint8_t> & wblk, const std::vector<float> & x, const char * what) {
    const int nb = K / 32;
    const size_t bsz = block_bytes(type);
    std::vector<int8_t> xq(K); std::vector<float> xd(nb), xs(nb);
    if (qref_quantize(0, x.data(), K, 1, nb, xq.data(), xd.data(), xs.data()) != 0) { printf("qref_quantize failed\n"); exit(2); }
    std::vector<uint8_t> y((size_t) nb * 34);
    q8_0(x.data(), y.data(), K);
    for (int b = 0; b < nb; ++b) {
        uint16_t dh; memcpy(&dh, &y[(size_t) b * 34], 2);
        if (!same(xd[b], wa_q1_h2f(dh)) || wa_q1_f2h(xd[b]) != dh) bad("q8_0 d", type, K, b, xd[b], wa_q1_h2f(dh));
        for (int e = 0; e < 32; ++e)
            if (xq[32 * b + e] != (int8_t) y[(size_t) b * 34 + 2 + e]) bad("q8_0 q", type, K, 32 * b + e, xq[32 * b + e], (int8_t) y[(size_t) b * 34 + 2 + e]);
        n_checked += 33;
    }
    std::vector<int8_t> wq((size_t) n_rows * K); std::vector<float> wd((size_t) n_rows * nb), want(n_rows), got(n_rows);
    for (int r = 0; r < n_rows; ++r) {
        const uint8_t * row = wblk.data() + (size_t) r * nb * bsz;
        for (int b = 0; b < nb; ++b) unpack(type, row + b * bsz, &wq[(size_t) r * K + 32 * b], wd[(size_t) r * nb + b]);
        (type == 6 ? dot5_0 : dot8_0)(K, &want[r], 0, row, 0, y.data(), 0, 1);
    }
    if (qref_gemm(0, 1, n_rows, nb, wq.data(), wd.data(), nullptr, xq.data(), xd.data(), nullptr, got.data()) != 0) { printf("qref_gemm failed\n"); exit(2); }
    for (int r = 0; r < n_rows; ++r) if (!same(got[r], want[r])) bad(what, type, K, r, got[r], want[r]);
    n_checked += n_rows;
}

int main(int argc, char ** argv) {
    if (argc < 2) { printf("usage: quant_ref_pin <reference library>\n"); return 2; }
    void * h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!h) { printf("cannot load %s: %s\n", argv[1], dlerror()); return 2; }
    q8_0 = (quant_fn) dlsym(h, "quantize_row_q8_0"); q5_0_ref = (quant_fn) dlsym(h, "quantize_row_q5_0_ref"); q8_0_ref = (quant_fn) dlsym(h, "quantize_row_q8_0_ref");
    dot5_0 = (dot_fn) dlsym(h, "ggml_vec_dot_q5_0_q8_0"); dot8_0 = (dot_fn) dlsym(h, "ggml_vec_dot_q8_0_q8_0");
    // ggml widens F16 through a table that its first initialisation fills
    if (void (*init)(void) = (void (*)(void)) dlsym(h, "ggml_cpu_init")) init(); else { printf("the reference library does not export ggml_cpu_init\n"); return 2; }
    if (!q8_0 || !q5_0_ref || !q8_0_ref || !dot5_0 || !dot8_0) { printf("the reference library does not export the quantisation functions\n"); return 2; }

    std::mt19937 rng(20240911);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    const int Ks[7] = { 32, 96, 128, 160, 384, 768, 3072 };
    for (int type : { 6, 8 }) {
        const size_t bsz = block_bytes(type);
        quant_fn wref = type == 6 ? q5_0_ref : q8_0_ref;
        for (int K : Ks) {
            const int nb = K / 32, R = 48;
            // (a) random weights quantised by the reference's own quantiser, random activation rows of several scales
            for (int rep = 0; rep < 6; ++rep) {
                std::vector<float> w((size_t) R * K), x(K);
                const float shift = rep % 3 == 0 ? 0.0f : rep % 3 == 1 ? 0.7f : -0.4f;
                for (auto & v : w) v = 0.05f * gauss(rng) + 0.02f * shift;
                const float xscale = rep < 2 ? 1.0f : rep < 4 ? 37.5f : 1e-3f;
                for (auto & v : x) v = xscale * (gauss(rng) + shift);
                std::vector<uint8_t> blk((size_t) R * nb * bsz);
                for (int r = 0; r < R; ++r) wref(&w[(size_t) r * K], &blk[(size_t) r * nb * bsz], K);
                check(type, K, R, blk, x, "dot");
            }
            // (b) raw blocks: every quant / high-bit pattern, scales drawn as F16 values of both signs over several binades, subnormal ones
            // and zeros included; for Q8_0 every third row holds bytes of -128 (the quantising tool never writes them)
            {
                std::vector<uint8_t> blk((size_t) R * nb * bsz);
                for (auto & v : blk) v = (uint8_t) (rng() & 0xff);
                for (size_t b = 0; b < (size_t) R * nb; ++b) {
                    const float dv = b % 7 == 0 ? 3e-6f * uni(rng) : b % 11 == 0 ? 0.0f : ldexpf(uni(rng), (int) (rng() % 12) - 8);
                    const uint16_t dh = wa_q1_f2h(dv);
                    memcpy(&blk[b * bsz], &dh, 2);
                    if (type == 8 && (b / nb) % 3 == 0) for (int e = 0; e < 32; e += 1 + (int) (rng() % 5)) blk[b * bsz + 2 + e] = 0x80;
                }
                std::vector<float> x(K);
                for (auto & v : x) v = 3.0f * gauss(rng);
                check(type, K, R, blk, x, "dot (raw blocks)");
                // saturated activations: every quant +-127 in alternating runs
                for (int i = 0; i < K; ++i) x[i] = (i / 4) & 1 ? -5.0f : 5.0f;
                check(type, K, R, blk, x, "dot (raw blocks, saturated row)");
                // (c) the rounding points of the activation row
                for (int b = 0; b < nb; ++b) for (int e = 0; e < 32; ++e) x[32 * b + e] = 0.0f;
                for (int b = 0; b < nb; ++b) {
                    float * xb = &x[32 * b];
                    switch ((b + 1) % 8) {                                                                // (K = 32: the one block holds ties)
                        case 0: break;                                                                          // an all-zero block: id = 0
                        case 1: xb[0] = 127.0f; for (int e = 1; e < 32; ++e) xb[e] = (float) (e - 16) + 0.5f; break;      // id = 1: every quant at a tie of rint
                        case 2: xb[0] = -254.0f; for (int e = 1; e < 32; ++e) xb[e] = (float) (2 * e - 31); break;        // id = 0.5: ties again, negative maximum
                        case 3: for (int e = 0; e < 32; ++e) xb[e] = 2047.0f; break;
                        case 4: for (int e = 0; e < 32; ++e) xb[e] = e == 7 ? -0.0f : 1e7f; break;              // d an F16 infinity, a -0.0 among the values
                        case 5: for (int e = 0; e < 32; ++e) xb[e] = -3000.0f; break;
                        case 6: for (int e = 0; e < 32; ++e) xb[e] = e & 1 ? 65000.0f : 64999.0f; break;
                        default: for (int e = 0; e < 32; ++e) xb[e] = 1e-7f * uni(rng); break;                  // d a subnormal half
                    }
                }
                check(type, K, R, blk, x, "dot (rounding points)");
            }
            // (d) weights far from zero, activations of mixed sign
            {
                std::vector<float> w((size_t) R * K), x(K);
                for (auto & v : w) v = 0.9f + 0.002f * gauss(rng);
                for (auto & v : x) v = 5.0f + gauss(rng);
                for (int i = 0; i < K; i += 3) x[i] = -x[i];
                std::vector<uint8_t> blk((size_t) R * nb * bsz);
                for (int r = 0; r < R; ++r) wref(&w[(size_t) r * K], &blk[(size_t) r * nb * bsz], K);
                check(type, K, R, blk, x, "dot (offset weights)");
            }
        }
    }
    printf("quant_ref: %ld values checked\n", n_checked);
    printf("quant_ref: %ld mismatches\n", n_bad);
    return n_bad == 0 ? 0 : 1;
}

// The host restatement of the Q4_1 / Q5_1 x Q8_1 arithmetic (whisper-rust_amd/csrc/wa_quant1.h: block unpack, dequantisation, Q8_1
// quantisation of a row with its block sums, one output of the product) against the reference library's own exported functions,
// bit for bit.  argv[1] = path of the reference library.  Prints "quant1: N mismatches" (N = 0 is the pass).
#include "wa_quant1.h"

#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef void (*quant_fn)(const float *, void *, int64_t);
typedef void (*dequant_fn)(const void *, float *, int64_t);
typedef void (*dot_fn)(int, float *, size_t, const void *, size_t, const void *, size_t, int);

static quant_fn q8_1, q4_1_ref, q5_1_ref;
static dequant_fn dq4_1, dq5_1;
static dot_fn dot4_1, dot5_1;
static long n_bad = 0, n_checked = 0;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
static void bad(const char * what, int type, int K, long i, float got, float want) {
    if (n_bad < 20) printf("MISMATCH %s type %d K %d at %ld: got %a (%08x) want %a (%08x)\n", what, type, K, i, got, bits(got), want, bits(want));
    n_bad += 1;
}

// weight rows given as raw blocks (type 3: 20 bytes each, type 7: 24) x one activation row: every function of the header against the reference's
static void check(int type, int K, int n_rows, const std::vector<uint8_t> & wblk, const std::vector<float> & x, const char * what) {
    const int nb = K / 32;
    const size_t bsz = wa_q1_block_bytes(type);
    // activation row: ours / the reference's block_q8_1 { f16 d; f16 s; i8 qs[32]; }
    std::vector<int8_t> xq(K); std::vector<float> xd(nb), xs(nb);
    wa_q8_1_row(x.data(), nb, xq.data(), xd.data(), xs.data());
    std::vector<uint8_t> y((size_t) nb * 36);
    q8_1(x.data(), y.data(), K);
    for (int b = 0; b < nb; ++b) {
        uint16_t dh, sh; memcpy(&dh, &y[(size_t) b * 36], 2); memcpy(&sh, &y[(size_t) b * 36 + 2], 2);
        if (!same(xd[b], wa_q1_h2f(dh)) || wa_q1_f2h(xd[b]) != dh) bad("q8_1 d", type, K, b, xd[b], wa_q1_h2f(dh));
        if (!same(xs[b], wa_q1_h2f(sh)) || (xs[b] == xs[b] && wa_q1_f2h(xs[b]) != sh)) bad("q8_1 s", type, K, b, xs[b], wa_q1_h2f(sh));
        for (int e = 0; e < 32; ++e)
            if (xq[32 * b + e] != (int8_t) y[(size_t) b * 36 + 4 + e]) bad("q8_1 q", type, K, 32 * b + e, xq[32 * b + e], (int8_t) y[(size_t) b * 36 + 4 + e]);
        n_checked += 34;
    }
    std::vector<int8_t> wq(K); std::vector<float> wd(nb), wm(nb), deq(K);
    for (int r = 0; r < n_rows; ++r) {
        const uint8_t * row = wblk.data() + (size_t) r * nb * bsz;
        for (int b = 0; b < nb; ++b) wa_q1_unpack(type, row + b * bsz, &wq[32 * b], wd[b], wm[b]);
        (type == 3 ? dq4_1 : dq5_1)(row, deq.data(), K);
        for (int i = 0; i < K; ++i) {
            const float got = wa_q1_dequant(wq[i], wd[i / 32], wm[i / 32]);
            if (!same(got, deq[i])) bad("dequant", type, K, i, got, deq[i]);
        }
        float want = 0.0f;
        (type == 3 ? dot4_1 : dot5_1)(K, &want, 0, row, 0, y.data(), 0, 1);
        const float got = wa_q1_dot(nb, wq.data(), wd.data(), wm.data(), xq.data(), xd.data(), xs.data());
        if (!same(got, want)) bad(what, type, K, r, got, want);
        n_checked += K + 1;
    }
}

int main(int argc, char ** argv) {
    if (argc < 2) { printf("usage: quant1_math <reference library>\n"); return 2; }
    void * h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!h) { printf("cannot load %s: %s\n", argv[1], dlerror()); return 2; }
    q8_1 = (quant_fn) dlsym(h, "quantize_row_q8_1"); q4_1_ref = (quant_fn) dlsym(h, "quantize_row_q4_1_ref"); q5_1_ref = (quant_fn) dlsym(h, "quantize_row_q5_1_ref");
    dq4_1 = (dequant_fn) dlsym(h, "dequantize_row_q4_1"); dq5_1 = (dequant_fn) dlsym(h, "dequantize_row_q5_1");
    dot4_1 = (dot_fn) dlsym(h, "ggml_vec_dot_q4_1_q8_1"); dot5_1 = (dot_fn) dlsym(h, "ggml_vec_dot_q5_1_q8_1");
    // ggml widens F16 through a table that its first initialisation fills
    if (void (*init)(void) = (void (*)(void)) dlsym(h, "ggml_cpu_init")) init(); else { printf("the reference library does not export ggml_cpu_init\n"); return 2; }
    if (!q8_1 || !q4_1_ref || !q5_1_ref || !dq4_1 || !dq5_1 || !dot4_1 || !dot5_1) { printf("the reference library does not export the quantisation functions\n"); return 2; }

    std::mt19937 rng(20240607);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    const int Ks[4] = { 128, 384, 768, 3072 };
    for (int type : { 3, 7 }) {
        const size_t bsz = wa_q1_block_bytes(type);
        quant_fn wref = type == 3 ? q4_1_ref : q5_1_ref;
        for (int K : Ks) {
            const int nb = K / 32, R = 48;
            // (a) random weights quantised by the reference's own quantiser (a shifted mean: minimums of both signs), random activation rows of several scales
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
            // (b) raw blocks: every quant / high-bit pattern, scales and minimums drawn as F16 values of both signs, subnormal ones included
            {
                std::vector<uint8_t> blk((size_t) R * nb * bsz);
                for (auto & v : blk) v = (uint8_t) (rng() & 0xff);
                for (size_t b = 0; b < (size_t) R * nb; ++b) {
                    const float dv = b % 7 == 0 ? 3e-6f * uni(rng) : 0.02f * uni(rng), mv = b % 5 == 0 ? 0.0f : 0.3f * uni(rng);
                    const uint16_t dh = wa_q1_f2h(dv), mh = wa_q1_f2h(mv);
                    memcpy(&blk[b * bsz], &dh, 2); memcpy(&blk[b * bsz + 2], &mh, 2);
                }
                std::vector<float> x(K);
                for (auto & v : x) v = 3.0f * gauss(rng);
                check(type, K, R, blk, x, "dot (raw blocks)");
                // (c) the rounding points of the activation row
                for (int b = 0; b < nb; ++b) for (int e = 0; e < 32; ++e) x[32 * b + e] = 0.0f;
                for (int b = 0; b < nb; ++b) {
                    float * xb = &x[32 * b];
                    switch (b % 8) {
                        case 0: break;                                                                          // an all-zero block: id = 0
                        case 1: xb[0] = 127.0f; for (int e = 1; e < 32; ++e) xb[e] = (float) (e - 16) + 0.5f; break;      // id = 1: every quant at a tie of rint
                        case 2: xb[0] = -254.0f; for (int e = 1; e < 32; ++e) xb[e] = (float) (2 * e - 31); break;        // id = 0.5: ties again, negative maximum
                        case 3: for (int e = 0; e < 32; ++e) xb[e] = 2047.0f; break;                            // s = d * 4064 close to the F16 limit 65504
                        case 4: for (int e = 0; e < 32; ++e) xb[e] = 2047.5f + 0.25f * (float) (b / 8); break;  // ... at the limit
                        case 5: for (int e = 0; e < 32; ++e) xb[e] = -3000.0f; break;                           // beyond it: what the F16 field of s holds
                        case 6: for (int e = 0; e < 32; ++e) xb[e] = e & 1 ? 65000.0f : 64999.0f; break;        // d itself stays finite, s does not
                        default: for (int e = 0; e < 32; ++e) xb[e] = 1e-7f * uni(rng); break;                  // d a subnormal half
                    }
                }
                check(type, K, R, blk, x, "dot (rounding points)");
            }
            // (d) summs and hsum far apart and of opposite sign: a swapped final addition or an fma in the chain moves the result by many ulps
            {
                std::vector<float> w((size_t) R * K), x(K);
                for (auto & v : w) v = 0.9f + 0.002f * gauss(rng);          // minimum ~ 0.89, scale tiny
                for (auto & v : x) v = 5.0f + gauss(rng);
                for (int i = 0; i < K; i += 3) x[i] = -x[i];
                std::vector<uint8_t> blk((size_t) R * nb * bsz);
                for (int r = 0; r < R; ++r) wref(&w[(size_t) r * K], &blk[(size_t) r * nb * bsz], K);
                check(type, K, R, blk, x, "dot (large minimum chain)");
            }
        }
    }
    printf("quant1: %ld values checked\n", n_checked);
    printf("quant1: %ld mismatches\n", n_bad);
    return n_bad == 0 ? 0 : 1;
}

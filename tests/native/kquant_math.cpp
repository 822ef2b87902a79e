// The host restatement of the Q5_K / Q6_K x Q8_K arithmetic (whisper-rust_amd/csrc/wa_quantk.h: block unpack, dequantisation, the Q8_K
// row with its sums, one output of either product) against the reference library's own exported functions, bit for bit, and the
// deliberately wrong variants of tests/native/kquant_ref.cpp, each of which must move some expected value on these rows.
// argv[1] = path of the reference library.  Prints "kquant: N mismatches" (N = 0 is the pass) and "kquant: variant ... changes M values".
#include "kquant_ref.cpp"
#include "wa_quant1.h"        // wa_q1_f2h: float -> IEEE half bits in integer arithmetic

#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <random>

typedef void (*quant_fn)(const float *, void *, int64_t);
typedef void (*dequant_fn)(const void *, float *, int64_t);
typedef void (*dot_fn)(int, float *, size_t, const void *, size_t, const void *, size_t, int);

static quant_fn q8_K, q5_K_ref, q6_K_ref;
static dequant_fn dq5_K, dq6_K;
static dot_fn dot5_K, dot6_K;
static long n_bad = 0, n_checked = 0;
// values a wrong variant moved: [0] last-index maximum, [1] swapped nibbles, [2] non-fused chain, [3] hsum order, [4] summs as fma, [5] summs added early
static long n_moved[6] = { 0, 0, 0, 0, 0, 0 };

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
static void bad(const char * what, int type, int K, long i, float got, float want) {
    if (n_bad < 20) printf("MISMATCH %s type %d K %d at %ld: got %a (%08x) want %a (%08x)\n", what, type, K, i, got, bits(got), want, bits(want));
    n_bad += 1;
}

#define Q8K_BYTES 292        // block_q8_K { f32 d; i8 qs[256]; i16 bsums[16]; }

// weight rows given as raw blocks x one activation row: every function of the header against the reference's
static void check(int type, int K, int n_rows, const std::vector<uint8_t> & wblk, const std::vector<float> & x, const char * what) {
    const int nb = K / 256;
    const size_t bsz = wa_qk_block_bytes(type);
    std::vector<int8_t> xq(K), xq1(K); std::vector<float> xd(nb), xd1(nb); std::vector<int16_t> xbs(16 * nb), xbs1(16 * nb);
    wa_q8_K_row(x.data(), nb, xq.data(), xd.data(), xbs.data());
    std::vector<uint8_t> y((size_t) nb * Q8K_BYTES);
    q8_K(x.data(), y.data(), K);
    for (int b = 0; b < nb; ++b) {
        const uint8_t * yb = &y[(size_t) b * Q8K_BYTES];
        float d; memcpy(&d, yb, 4);
        if (!same(xd[b], d)) bad("q8_K d", type, K, b, xd[b], d);
        for (int e = 0; e < 256; ++e) if (xq[256 * b + e] != (int8_t) yb[4 + e]) bad("q8_K q", type, K, 256 * b + e, xq[256 * b + e], (int8_t) yb[4 + e]);
        if (d != 0.0f)            // (the reference leaves the sums of an all-zero block unwritten)
            for (int j = 0; j < 16; ++j) { int16_t s; memcpy(&s, yb + 260 + 2 * j, 2); if (s != xbs[16 * b + j]) bad("q8_K bsums", type, K, 16 * b + j, xbs[16 * b + j], s); }
        n_checked += 273;
    }
    kq_q8_K_row(x.data(), nb, xq1.data(), xd1.data(), xbs1.data(), 1);
    for (int b = 0; b < nb; ++b) if (!same(xd[b], xd1[b])) n_moved[0] += 1;
    std::vector<int8_t> wq(K), wsc(16 * nb), wq1(K), wsc1(16 * nb); std::vector<float> wd(nb), wdm(nb), wd1(nb), wdm1(nb), deq(K);
    for (int r = 0; r < n_rows; ++r) {
        const uint8_t * row = wblk.data() + (size_t) r * nb * bsz;
        for (int b = 0; b < nb; ++b) {
            wa_qk_unpack(type, row + b * bsz, &wq[256 * b], &wsc[16 * b], wd[b], wdm[b]);
            kq_unpack_block(type, row + b * bsz, &wq1[256 * b], &wsc1[16 * b], wd1[b], wdm1[b], 1);
        }
        (type == WA_TYPE_Q5_K ? dq5_K : dq6_K)(row, deq.data(), K);
        for (int i = 0; i < K; ++i) {
            const float got = wa_qk_dequant(type, &wq[i & ~255], &wsc[16 * (i >> 8)], wd[i >> 8], wdm[i >> 8], i & 255);
            if (!same(got, deq[i])) bad("dequant", type, K, i, got, deq[i]);
        }
        float want = 0.0f;
        (type == WA_TYPE_Q5_K ? dot5_K : dot6_K)(K, &want, 0, row, 0, y.data(), 0, 1);
        const float got = wa_qk_dot(type, nb, wq.data(), wsc.data(), wd.data(), wdm.data(), xq.data(), xd.data(), xbs.data());
        if (!same(got, want)) bad(what, type, K, r, got, want);
        n_checked += K + 1;
        if (!same(wa_qk_dot(type, nb, wq1.data(), wsc1.data(), wd1.data(), wdm1.data(), xq.data(), xd.data(), xbs.data()), want)) n_moved[1] += 1;
        for (int v = 1; v <= 4; ++v)
            if (!same(kq_dot(type, nb, wq.data(), wsc.data(), wd.data(), wdm.data(), xq.data(), xd.data(), xbs.data(), v), want)) n_moved[1 + v] += 1;
    }
}

int main(int argc, char ** argv) {
    if (argc < 2) { printf("usage: kquant_math <reference library>\n"); return 2; }
    void * h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!h) { printf("cannot load %s: %s\n", argv[1], dlerror()); return 2; }
    q8_K = (quant_fn) dlsym(h, "quantize_row_q8_K"); q5_K_ref = (quant_fn) dlsym(h, "quantize_row_q5_K_ref"); q6_K_ref = (quant_fn) dlsym(h, "quantize_row_q6_K_ref");
    dq5_K = (dequant_fn) dlsym(h, "dequantize_row_q5_K"); dq6_K = (dequant_fn) dlsym(h, "dequantize_row_q6_K");
    dot5_K = (dot_fn) dlsym(h, "ggml_vec_dot_q5_K_q8_K"); dot6_K = (dot_fn) dlsym(h, "ggml_vec_dot_q6_K_q8_K");
    // ggml widens F16 through a table that its first initialisation fills
    if (void (*init)(void) = (void (*)(void)) dlsym(h, "ggml_cpu_init")) init(); else { printf("the reference library does not export ggml_cpu_init\n"); return 2; }
    if (!q8_K || !q5_K_ref || !q6_K_ref || !dq5_K || !dq6_K || !dot5_K || !dot6_K) { printf("the reference library does not export the K-format functions\n"); return 2; }

    std::mt19937 rng(20240913);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    const int Ks[6] = { 256, 512, 768, 1024, 3072, 5120 };
    for (int type : { WA_TYPE_Q5_K, WA_TYPE_Q6_K }) {
        const size_t bsz = wa_qk_block_bytes(type);
        quant_fn wref = type == WA_TYPE_Q5_K ? q5_K_ref : q6_K_ref;
        for (int K : Ks) {
            const int nb = K / 256, R = 24;
            // (a) random weights quantised by the reference's own quantiser (a shifted mean: Q5_K minimums in use), activation rows of several scales
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
            // (b) raw blocks: every quant / high-bit / scale-byte pattern, d and dmin drawn as F16 values of both signs, subnormal ones included
            std::vector<uint8_t> blk((size_t) R * nb * bsz);
            for (auto & v : blk) v = (uint8_t) (rng() & 0xff);
            for (size_t b = 0; b < (size_t) R * nb; ++b) {
                const float dv = b % 7 == 0 ? 3e-6f * uni(rng) : 0.002f * uni(rng), mv = b % 5 == 0 ? 0.0f : 0.01f * uni(rng);
                const uint16_t dh = wa_q1_f2h(dv), mh = wa_q1_f2h(mv);
                if (type == WA_TYPE_Q5_K) { memcpy(&blk[b * bsz], &dh, 2); memcpy(&blk[b * bsz + 2], &mh, 2); }
                else memcpy(&blk[b * bsz + 208], &dh, 2);
            }
            std::vector<float> x(K);
            for (auto & v : x) v = 3.0f * gauss(rng);
            check(type, K, R, blk, x, "dot (raw blocks)");
            // (c) the rounding points of the activation row, one kind per block, the kinds rotating with K so that every width meets several
            for (int b = 0; b < nb; ++b) {
                float * xb = &x[256 * b];
                for (int e = 0; e < 256; ++e) xb[e] = 0.25f * gauss(rng);
                switch ((b + K / 256) % 8) {
                    case 0: for (int e = 0; e < 256; ++e) xb[e] = 0.0f; break;                                   // an all-zero block: d = 0, quants 0
                    case 1: xb[3] = 5.0f; xb[100] = -5.0f; break;                                                // equal maxima, + first: the scale is negative
                    case 2: xb[7] = -5.0f; xb[8] = 5.0f; xb[255] = -5.0f; break;                                 // ... - first, three holders
                    case 3: for (int e = 0; e < 256; ++e) xb[e] = (float) (e % 120) + 0.5f; xb[17] = -127.0f; break;     // iscale = 1: every product at a tie of nearest_int
                    case 4: for (int e = 0; e < 256; ++e) xb[e] = (float) (2 * (e % 127) - 125); xb[200] = 254.0f; break; // iscale = -0.5: ties, positive maximum
                    case 5: for (int e = 0; e < 256; ++e) xb[e] = -fabsf(xb[e]); xb[255] = -9.0f; break;         // a negative maximum in the last element
                    case 6: for (int e = 0; e < 256; ++e) xb[e] = e & 1 ? 3.0f : -3.0f; break;                   // every element a holder: the first one (+... -3) decides
                    default: for (int e = 0; e < 256; ++e) xb[e] = 1e-30f * uni(rng); break;                     // 1 / iscale far down the exponent range
                }
            }
            check(type, K, R, blk, x, "dot (rounding points)");
            // (d) a large minimum chain against small lane sums, opposite signs: the place of the summs addition and its rounding show
            {
                std::vector<float> w((size_t) R * K), xx(K);
                for (auto & v : w) v = 0.9f + 0.002f * gauss(rng);
                for (auto & v : xx) v = 5.0f + gauss(rng);
                for (int i = 0; i < K; i += 3) xx[i] = -xx[i];
                std::vector<uint8_t> blk2((size_t) R * nb * bsz);
                for (int r = 0; r < R; ++r) wref(&w[(size_t) r * K], &blk2[(size_t) r * nb * bsz], K);
                check(type, K, R, blk2, xx, "dot (large minimum chain)");
            }
        }
    }
    const char * names[6] = { "last-index maximum", "swapped nibble halves", "non-fused chain", "other hsum order", "summs as one fma", "summs added early" };
    for (int v = 0; v < 6; ++v) printf("kquant: variant %s changes %ld values\n", names[v], n_moved[v]);
    printf("kquant: %ld values checked\n", n_checked);
    printf("kquant: %ld mismatches\n", n_bad);
    bool all_moved = true;
    for (int v = 0; v < 6; ++v) all_moved = all_moved && n_moved[v] > 0;
    if (!all_moved) printf("kquant: a wrong variant changed nothing\n");
    return n_bad == 0 && all_moved ? 0 : 1;
}

// The host restatement of the Q2_K / Q3_K x Q8_K arithmetic (whisper-rust_amd/csrc/wa_quantk.h: block unpack, dequantisation, one output
// of either product) against the reference library's own exported functions, bit for bit, and deliberately wrong variants, each of which
// must move some expected value on these rows - or the rows that pin it are missing:
//   Q2_K   the minimum term after the product term | the minimums as a scalar chain added after hsum | the minimum fma as a multiplication
//          and an addition | the product fma likewise | scale and minimum nibbles swapped
//   Q3_K   the high-bit polarity inverted | the two upper scale bits taken from the wrong byte
//   both   hsum_float_8 in lane order
// argv[1] = path of the reference library.  Prints "kquant23: N mismatches" (N = 0 is the pass) and "kquant23: variant ... changes M values".
#include "wa_quantk.h"
#include "wa_quant1.h"        // wa_q1_f2h: float -> IEEE half bits in integer arithmetic

#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

typedef void (*quant_fn)(const float *, void *, int64_t);
typedef void (*dequant_fn)(const void *, float *, int64_t);
typedef void (*dot_fn)(int, float *, size_t, const void *, size_t, const void *, size_t, int);
struct init_params { size_t mem_size; void * mem_buffer; bool no_alloc; };        // ggml_init_params

static quant_fn q8_K, q2_K_ref, q3_K_ref;
static dequant_fn dq2_K, dq3_K;
static dot_fn dot2_K, dot3_K;
static long n_bad = 0, n_checked = 0;

enum { V_MIN_AFTER, V_MIN_SCALAR, V_MIN_NOFMA, V_PROD_NOFMA, V_NIBBLES, V_HMASK, V_SCALE_HI, V_HSUM_Q2, V_HSUM_Q3, N_VARIANTS };
static const char * names[N_VARIANTS] = { "Q2_K minimum term after the product term", "Q2_K minimums as a scalar chain", "Q2_K minimum term not fused",
                                          "Q2_K product term not fused", "Q2_K swapped scale nibbles", "Q3_K inverted high bit", "Q3_K upper scale bits of the wrong byte",
                                          "Q2_K other hsum order", "Q3_K other hsum order" };
static long n_moved[N_VARIANTS];

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }
static void bad(const char * what, int type, int K, long i, float got, float want) {
    if (n_bad < 20) printf("MISMATCH %s type %d K %d at %ld: got %a (%08x) want %a (%08x)\n", what, type, K, i, got, bits(got), want, bits(want));
    n_bad += 1;
}

#define Q8K_BYTES 292        // block_q8_K { f32 d; i8 qs[256]; i16 bsums[16]; }

// a block with one thing wrong in it, for the variants that are wrong in the unpack
static void wrong_block(int variant, const uint8_t * blk, size_t bsz, uint8_t * out) {
    memcpy(out, blk, bsz);
    if (variant == V_NIBBLES) for (int i = 0; i < 16; ++i) out[i] = (uint8_t) ((blk[i] >> 4) | (blk[i] << 4));
    if (variant == V_HMASK)   for (int i = 0; i < 32; ++i) out[i] = (uint8_t) ~blk[i];
    if (variant == V_SCALE_HI) for (int i = 0; i < 4; ++i) out[96 + 8 + i] = blk[96 + 8 + ((i + 1) & 3)];
}

// wa_qk_dot with one thing wrong in the order
static float dot_variant(int variant, int type, int nb, const int8_t * wq, const int8_t * wsc, const float * wd, const float * wdmin, const int8_t * xq,
                         const float * xd, const int16_t * xbs) {
    float acc[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    float chain = 0.0f;
    for (int b = 0; b < nb; ++b) {
        const float dd = xd[b] * wd[b], dn = -xd[b] * wdmin[b];
        int sumi[8], mins[8];
        for (int l = 0; l < 8; ++l) {
            sumi[l] = 0;
            for (int g = 0; g < 8; ++g) {
                int sum4 = 0;
                for (int e = 0; e < 4; ++e) sum4 += (int) wq[256 * b + 32 * g + 4 * l + e] * (int) xq[256 * b + 32 * g + 4 * l + e];
                sumi[l] += wa_qk_scale_of(type, wsc + 16 * b, 32 * g + 4 * l) * sum4;
            }
            mins[l] = wa_qk_min_of(type, wsc + 16 * b, 32 * l) * (int) xbs[16 * b + 2 * l] + wa_qk_min_of(type, wsc + 16 * b, 32 * l + 16) * (int) xbs[16 * b + 2 * l + 1];
        }
        const bool q2 = type == WA_TYPE_Q2_K;
        if (q2 && variant == V_MIN_SCALAR) {
            int s = 0; for (int l = 0; l < 8; ++l) s += mins[l];
            chain = fmaf(dn, (float) s, chain);
        }
        for (int l = 0; l < 8; ++l) {
            if (q2 && variant != V_MIN_AFTER && variant != V_MIN_SCALAR) {
                if (variant == V_MIN_NOFMA) { const float p = dn * (float) mins[l]; acc[l] = acc[l] + p; }
                else acc[l] = fmaf(dn, (float) mins[l], acc[l]);
            }
            if (variant == V_PROD_NOFMA) { const float p = dd * (float) sumi[l]; acc[l] = acc[l] + p; }
            else acc[l] = fmaf(dd, (float) sumi[l], acc[l]);
            if (q2 && variant == V_MIN_AFTER) acc[l] = fmaf(dn, (float) mins[l], acc[l]);
        }
    }
    float v;
    if (variant == V_HSUM_Q2 || variant == V_HSUM_Q3) { v = acc[0]; for (int l = 1; l < 8; ++l) v = v + acc[l]; }
    else v = wa_qk_hsum8(acc);
    return variant == V_MIN_SCALAR ? v + chain : v;
}

// weight rows given as raw blocks x one activation row: the header's unpack, dequantisation and product against the reference's
static void check(int type, int K, int n_rows, const std::vector<uint8_t> & wblk, const std::vector<float> & x, const char * what) {
    const int nb = K / 256;
    const size_t bsz = wa_qk_block_bytes(type);
    std::vector<int8_t> xq(K); std::vector<float> xd(nb); std::vector<int16_t> xbs(16 * nb);
    wa_q8_K_row(x.data(), nb, xq.data(), xd.data(), xbs.data());
    std::vector<uint8_t> y((size_t) nb * Q8K_BYTES);
    q8_K(x.data(), y.data(), K);
    for (int b = 0; b < nb; ++b) {        // (tests/native/kquant_math.cpp holds the Q8_K row itself; here only that both sides multiply the same row)
        float d; memcpy(&d, &y[(size_t) b * Q8K_BYTES], 4);
        if (!same(xd[b], d) || memcmp(&xq[256 * b], &y[(size_t) b * Q8K_BYTES + 4], 256) != 0) bad("q8_K row", type, K, b, xd[b], d);
    }
    std::vector<int8_t> wq(K), wsc(16 * nb), wq1(K), wsc1(16 * nb); std::vector<float> wd(nb), wdm(nb), wd1(nb), wdm1(nb), deq(K);
    std::vector<uint8_t> wrong(bsz);
    const bool q2 = type == WA_TYPE_Q2_K;
    for (int r = 0; r < n_rows; ++r) {
        const uint8_t * row = wblk.data() + (size_t) r * nb * bsz;
        for (int b = 0; b < nb; ++b) wa_qk_unpack(type, row + b * bsz, &wq[256 * b], &wsc[16 * b], wd[b], wdm[b]);
        (q2 ? dq2_K : dq3_K)(row, deq.data(), K);
        for (int i = 0; i < K; ++i) {
            const float got = wa_qk_dequant(type, &wq[i & ~255], &wsc[16 * (i >> 8)], wd[i >> 8], wdm[i >> 8], i & 255);
            if (!same(got, deq[i])) bad("dequant", type, K, i, got, deq[i]);
        }
        float want = 0.0f;
        (q2 ? dot2_K : dot3_K)(K, &want, 0, row, 0, y.data(), 0, 1);
        const float got = wa_qk_dot(type, nb, wq.data(), wsc.data(), wd.data(), wdm.data(), xq.data(), xd.data(), xbs.data());
        if (!same(got, want)) bad(what, type, K, r, got, want);
        if (!q2) {        // Q3_K, unpacked, IS a Q6_K row: the same function on the same arrays
            const float as6 = wa_qk_dot(WA_TYPE_Q6_K, nb, wq.data(), wsc.data(), wd.data(), wdm.data(), xq.data(), xd.data(), xbs.data());
            if (!same(as6, want)) bad("dot as Q6_K", type, K, r, as6, want);
        }
        n_checked += K + 1;
        for (int v = 0; v < N_VARIANTS; ++v) {
            const bool for_q2 = v <= V_NIBBLES || v == V_HSUM_Q2;
            if (for_q2 != q2) continue;
            float r1;
            if (v == V_NIBBLES || v == V_HMASK || v == V_SCALE_HI) {
                for (int b = 0; b < nb; ++b) {
                    wrong_block(v, row + b * bsz, bsz, wrong.data());
                    wa_qk_unpack(type, wrong.data(), &wq1[256 * b], &wsc1[16 * b], wd1[b], wdm1[b]);
                }
                r1 = wa_qk_dot(type, nb, wq1.data(), wsc1.data(), wd1.data(), wdm1.data(), xq.data(), xd.data(), xbs.data());
            } else r1 = dot_variant(v, type, nb, wq.data(), wsc.data(), wd.data(), wdm.data(), xq.data(), xd.data(), xbs.data());
            if (!same(r1, want)) n_moved[v] += 1;
        }
    }
}

int main(int argc, char ** argv) {
    if (argc < 2) { printf("usage: kquant23_math <reference library>\n"); return 2; }
    void * h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!h) { printf("cannot load %s: %s\n", argv[1], dlerror()); return 2; }
    // ggml widens F16 through a table that its first initialisation fills: before anything else
    void * (*init)(init_params) = (void * (*)(init_params)) dlsym(h, "ggml_init");
    if (!init) { printf("the reference library does not export ggml_init\n"); return 2; }
    void * gctx = init(init_params{ 1 << 20, nullptr, false });
    if (!gctx) { printf("ggml_init failed\n"); return 2; }
    if (void (*cpu_init)(void) = (void (*)(void)) dlsym(h, "ggml_cpu_init")) cpu_init();
    q8_K = (quant_fn) dlsym(h, "quantize_row_q8_K"); q2_K_ref = (quant_fn) dlsym(h, "quantize_row_q2_K_ref"); q3_K_ref = (quant_fn) dlsym(h, "quantize_row_q3_K_ref");
    dq2_K = (dequant_fn) dlsym(h, "dequantize_row_q2_K"); dq3_K = (dequant_fn) dlsym(h, "dequantize_row_q3_K");
    dot2_K = (dot_fn) dlsym(h, "ggml_vec_dot_q2_K_q8_K"); dot3_K = (dot_fn) dlsym(h, "ggml_vec_dot_q3_K_q8_K");
    if (!q8_K || !q2_K_ref || !q3_K_ref || !dq2_K || !dq3_K || !dot2_K || !dot3_K) { printf("the reference library does not export the K-format functions\n"); return 2; }

    std::mt19937 rng(20241019);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    const int Ks[5] = { 256, 512, 768, 1024, 5120 };
    for (int type : { WA_TYPE_Q2_K, WA_TYPE_Q3_K }) {
        const size_t bsz = wa_qk_block_bytes(type);
        const bool q2 = type == WA_TYPE_Q2_K;
        quant_fn wref = q2 ? q2_K_ref : q3_K_ref;
        for (int K : Ks) {
            const int nb = K / 256, R = 24;
            // (a) random weights quantised by the reference's own quantiser (a shifted mean: the Q2_K minimums in use), activation rows of several scales
            for (int rep = 0; rep < 6; ++rep) {
                std::vector<float> w((size_t) R * K), x(K);
                const float shift = rep % 3 == 0 ? 0.0f : rep % 3 == 1 ? 0.7f : -0.4f;
                for (auto & v : w) v = 0.05f * gauss(rng) + 0.02f * shift;
                for (int r = 0; r < R; r += 5) for (int e = 0; e < 256; ++e) w[(size_t) r * K + e] = 0.0f;       // zero weight blocks
                const float xscale = rep < 2 ? 1.0f : rep < 4 ? 37.5f : 1e-3f;
                for (auto & v : x) v = xscale * (gauss(rng) + shift);
                std::vector<uint8_t> blk((size_t) R * nb * bsz);
                for (int r = 0; r < R; ++r) wref(&w[(size_t) r * K], &blk[(size_t) r * nb * bsz], K);
                check(type, K, R, blk, x, "dot");
            }
            // (b) raw blocks: every quant / high-bit / scale pattern, d and dmin drawn as F16 values of both signs, subnormal and zero ones included
            std::vector<uint8_t> blk((size_t) R * nb * bsz);
            for (auto & v : blk) v = (uint8_t) (rng() & 0xff);
            for (size_t b = 0; b < (size_t) R * nb; ++b) {
                const float dv = b % 7 == 0 ? 3e-6f * uni(rng) : b % 11 == 0 ? 0.0f : 0.002f * uni(rng), mv = b % 5 == 0 ? 0.0f : 0.01f * uni(rng);
                const uint16_t dh = wa_q1_f2h(dv), mh = wa_q1_f2h(mv);
                if (q2) { memcpy(&blk[b * bsz + 80], &dh, 2); memcpy(&blk[b * bsz + 82], &mh, 2); }
                else memcpy(&blk[b * bsz + 108], &dh, 2);
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
            // (d) large minimum terms against small lane sums, opposite signs: the place of the minimum term and its rounding show
            {
                std::vector<float> w((size_t) R * K), xx(K);
                for (auto & v : w) v = 0.9f + 0.002f * gauss(rng);
                for (auto & v : xx) v = 5.0f + gauss(rng);
                for (int i = 0; i < K; i += 3) xx[i] = -xx[i];
                std::vector<uint8_t> blk2((size_t) R * nb * bsz);
                for (int r = 0; r < R; ++r) wref(&w[(size_t) r * K], &blk2[(size_t) r * nb * bsz], K);
                check(type, K, R, blk2, xx, "dot (large minimums)");
            }
        }
    }
    if (void (*gfree)(void *) = (void (*)(void *)) dlsym(h, "ggml_free")) gfree(gctx);
    for (int v = 0; v < N_VARIANTS; ++v) printf("kquant23: variant %s changes %ld values\n", names[v], n_moved[v]);
    printf("kquant23: %ld values checked\n", n_checked);
    printf("kquant23: %ld mismatches\n", n_bad);
    bool all_moved = true;
    for (int v = 0; v < N_VARIANTS; ++v) all_moved = all_moved && n_moved[v] > 0;
    if (!all_moved) printf("kquant23: a wrong variant changed nothing\n");
    return n_bad == 0 && all_moved ? 0 : 1;
}

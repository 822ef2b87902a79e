// The host statement of the Q4_0 and Q4_K arithmetic (whisper-rust_amd/csrc/wa_quant4.h) against the reference library, bit for bit: one-node MUL_MAT
// graphs whose weight lies in the reference's CPU repack buffer type (N % 8 == 0: the library itself picks quantiser, interleave and gemv / gemm) or in
// its plain CPU buffer (N = 9: ggml_vec_dot_q4_0_q8_0 / q4_K_q8_K), and dequantize_row_q4_0 / q4_K.  Rows 0 and M - 1 of the activations hold the quantisers'
// rounding points: an all-zero block, a block of rint ties, and a block with - m before + m - in a row below M - M % 4 once M >= 4 (the four-row quantiser's
// sign rule) and in the last row (a leftover row unless M % 4 == 0).  argv[1] = path of the reference library.  Prints "quant4: N mismatches" (0 is the pass).
#include "wa_quant4.h"

#include <dlfcn.h>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

struct init_params { size_t mem_size; void * mem_buffer; bool no_alloc; };       // ggml_init_params
static void * (*g_init)(init_params);
static void (*g_free)(void *);
static void * (*g_new_2d)(void *, int, int64_t, int64_t);
static void * (*g_mul_mat)(void *, void *, void *);
static void * (*g_new_graph)(void *);
static void (*g_expand)(void *, void *);
static size_t (*g_tensor_overhead)(void), (*g_graph_overhead)(void);
static void * (*g_alloc_buft)(void *, void *), * (*g_alloc)(void *, void *), * (*g_cpu_buft)(void), * (*g_repack_buft)(void);
static void (*g_set)(void *, const void *, size_t, size_t);
static void (*g_get)(const void *, void *, size_t, size_t);
static int (*g_compute)(void *, void *);
static void (*g_buf_free)(void *);
static void (*q_ref[2])(const float *, void *, int64_t);        // quantize_row_q4_0_ref, q4_K_ref
static void (*dq[2])(const void *, float *, int64_t);           // dequantize_row_q4_0, q4_K
static void * backend;
static long n_bad = 0, n_checked = 0;

static void cmp(const char * what, int k, int M, int N, int K, long i, float got, float want) {
    n_checked += 1;
    if (memcmp(&got, &want, 4) == 0) return;
    if (n_bad < 20) printf("MISMATCH %s %s M %d N %d K %d at %ld: got %a want %a\n", k ? "q4_K" : "q4_0", what, M, N, K, i, got, want);
    n_bad += 1;
}

// the library's x W^T: W raw blocks of ggml `type` [N][K], x f32 [M][K] -> out [M][N]
static void ref_mul_mat(int type, const std::vector<uint8_t> & blk, int N, int K, const std::vector<float> & x, int M, bool repack, std::vector<float> & out) {
    void * cw = g_init({ 4 * g_tensor_overhead(), nullptr, true });
    void * W = g_new_2d(cw, type, K, N);
    void * bw = g_alloc_buft(cw, repack ? g_repack_buft() : g_cpu_buft());
    g_set(W, blk.data(), 0, blk.size());
    void * cc = g_init({ 8 * g_tensor_overhead() + g_graph_overhead(), nullptr, true });
    void * X = g_new_2d(cc, 0, K, M);
    void * Y = g_mul_mat(cc, W, X);
    void * gf = g_new_graph(cc);
    g_expand(gf, Y);
    void * bc = g_alloc(cc, backend);
    g_set(X, x.data(), 0, x.size() * 4);
    if (g_compute(backend, gf) != 0) { printf("graph compute failed\n"); exit(2); }
    out.resize((size_t) M * N);
    g_get(Y, out.data(), 0, out.size() * 4);
    g_buf_free(bc); g_buf_free(bw); g_free(cc); g_free(cw);
}

// k: Q4_K, else Q4_0.  The kernel layout must hold the unpacked values (N % 8 == 0), the dequantised row the library's (N = 9), every output the library's.
static void check(int k, const std::vector<uint8_t> & blk, int N, int K, const std::vector<float> & x, int M, const char * what) {
    const int per = k ? 256 : 32, nb = K / per, bsz = k ? WA_Q4_K_BYTES : WA_Q4_0_BYTES, n4 = k ? wa_q4_K_rows4(M) : 0;
    const bool inter = N % 8 == 0;
    std::vector<float> want;
    ref_mul_mat(k ? WA_TYPE_Q4_K : WA_TYPE_Q4_0, blk, N, K, x, M, inter, want);
    std::vector<int8_t> xq((size_t) M * K), wq(K); std::vector<float> xd((size_t) M * nb), wd(nb), wdm(nb), deq(K); std::vector<int16_t> xbs((size_t) M * K / 16);
    std::vector<uint8_t> wsc(K / 16), packed((size_t) N * K / 2), psc((size_t) N * K / 16); std::vector<float> pd((size_t) N * nb), pm((size_t) N * nb);
    for (int m = 0; m < M; ++m)          // Q4_K, interleaved: rows below M - M % 4 by the four-row quantiser; else the row quantiser
        if (k) (inter && m < n4 ? wa_q8_K_row4 : wa_q8_K_row)(&x[(size_t) m * K], nb, &xq[(size_t) m * K], &xd[(size_t) m * nb], &xbs[(size_t) m * nb * 16]);
        else wa_q8_0_row(&x[(size_t) m * K], nb, &xq[(size_t) m * K], &xd[(size_t) m * nb]);
    if (k) wa_q4_K_pack_rows(blk.data(), N, nb, packed.data(), psc.data(), pd.data(), pm.data()); else wa_q4_0_pack_rows(blk.data(), N, nb, packed.data(), pd.data());
    for (int n = 0; n < N; ++n) {
        const uint8_t * row = blk.data() + (size_t) n * nb * bsz;
        for (int b = 0; b < nb; ++b)
            if (k) wa_q4_K_unpack(row + b * bsz, &wq[256 * b], &wsc[16 * b], wd[b], wdm[b]); else wa_q4_0_unpack(row + b * bsz, &wq[32 * b], wd[b]);
        if (inter) {
            for (int i = 0; i < K; ++i) cmp("layout", k, M, N, K, i, (float) (k ? wa_q4_K_packed_at(packed.data(), n, nb, i >> 8, i & 255) : wa_q4_0_packed_at(packed.data(), n, nb, i >> 5, i & 31)), (float) wq[i]);
            for (int b = 0; b < nb; ++b) { cmp("layout d", k, M, N, K, b, pd[(size_t) n * nb + b], wd[b]); if (k) cmp("layout dmin", k, M, N, K, b, pm[(size_t) n * nb + b], wdm[b]); }
            for (int i = 0; k && i < 16 * nb; ++i) cmp("layout scales", k, M, N, K, i, (float) psc[(size_t) n * nb * 16 + i], (float) wsc[i]);
        } else {
            dq[k](row, deq.data(), K);
            for (int i = 0; i < K; ++i)
                cmp("dequant", k, M, N, K, i, k ? wa_qk_dequant(WA_TYPE_Q5_K, &wq[i & ~255], (const int8_t *) &wsc[16 * (i >> 8)], wd[i >> 8], wdm[i >> 8], i & 255) : wa_q4_0_dequant(wq[i], wd[i >> 5]), deq[i]);
        }
        for (int m = 0; m < M; ++m) {
            const int8_t * q = &xq[(size_t) m * K]; const float * d = &xd[(size_t) m * nb]; const int16_t * bs = &xbs[(size_t) m * (k ? nb * 16 : 0)];
            const float got = k ? (inter ? wa_q4_K_dot8(nb, wq.data(), wsc.data(), wd.data(), wdm.data(), q, d, bs, m < n4) : wa_q4_K_dot_plain(nb, wq.data(), wsc.data(), wd.data(), wdm.data(), q, d, bs))
                                : (inter ? wa_q4_0_dot8(nb, wq.data(), wd.data(), q, d) : wa_q4_0_dot_plain(nb, wq.data(), wd.data(), q, d));
            cmp(what, k, M, N, K, (long) m * N + n, got, want[(size_t) m * N + n]);
        }
    }
}

#define SYM(var, name) do { *(void **) &var = dlsym(h, name); if (!var) { printf("the reference library does not export %s\n", name); return 2; } } while (0)
int main(int argc, char ** argv) {
    if (argc < 2) { printf("usage: quant4_math <reference library>\n"); return 2; }
    void * h = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!h) { printf("cannot load %s: %s\n", argv[1], dlerror()); return 2; }
    void (*cpu_init)(void); void * (*backend_init)(void); void (*set_threads)(void *, int);
    SYM(cpu_init, "ggml_cpu_init"); SYM(backend_init, "ggml_backend_cpu_init"); SYM(set_threads, "ggml_backend_cpu_set_n_threads");
    SYM(g_init, "ggml_init"); SYM(g_free, "ggml_free"); SYM(g_new_2d, "ggml_new_tensor_2d"); SYM(g_mul_mat, "ggml_mul_mat"); SYM(g_new_graph, "ggml_new_graph");
    SYM(g_expand, "ggml_build_forward_expand"); SYM(g_tensor_overhead, "ggml_tensor_overhead"); SYM(g_graph_overhead, "ggml_graph_overhead");
    SYM(g_alloc_buft, "ggml_backend_alloc_ctx_tensors_from_buft"); SYM(g_alloc, "ggml_backend_alloc_ctx_tensors"); SYM(g_set, "ggml_backend_tensor_set");
    SYM(g_get, "ggml_backend_tensor_get"); SYM(g_compute, "ggml_backend_graph_compute"); SYM(g_cpu_buft, "ggml_backend_cpu_buffer_type");
    SYM(g_repack_buft, "_Z35ggml_backend_cpu_repack_buffer_typev"); SYM(g_buf_free, "ggml_backend_buffer_free");
    SYM(q_ref[0], "quantize_row_q4_0_ref"); SYM(dq[0], "dequantize_row_q4_0"); SYM(q_ref[1], "quantize_row_q4_K_ref"); SYM(dq[1], "dequantize_row_q4_K");
    cpu_init();
    backend = backend_init();
    set_threads(backend, 3);           // the library splits rows of W and groups of four rows of x over its threads: the values must not depend on it

    std::mt19937 rng(20241126);
    std::normal_distribution<float> gauss(0.0f, 1.0f);
    std::uniform_real_distribution<float> uni(-1.0f, 1.0f);
    for (int k = 0; k < 2; ++k)
        for (int N : { 16, 9 })
            for (int K : (k ? std::vector<int>{ 256, 768 } : std::vector<int>{ 32, 96, 768 })) {
                const int per = k ? 256 : 32, nb = K / per, bsz = k ? WA_Q4_K_BYTES : WA_Q4_0_BYTES;
                // (a) weights quantised by the library's own quantiser: block scales over five decades, a shifted mean (Q4_K's minimums in use)
                std::vector<float> w((size_t) N * K);
                for (size_t i = 0; i < w.size(); ++i) w[i] = (gauss(rng) + ((i / 32) % 3 == 0 ? 0.8f : -0.3f)) * powf(10.0f, -3.0f + (float) ((i / per) % 6));
                std::vector<uint8_t> blk((size_t) N * nb * bsz), raw(blk.size());
                for (int n = 0; n < N; ++n) q_ref[k](&w[(size_t) n * K], &blk[(size_t) n * nb * bsz], K);
                // (b) raw blocks: every nibble (and 6-bit scale / minimum) pattern, d (and dmin) drawn as F16 values of both signs, subnormal ones included
                for (auto & v : raw) v = (uint8_t) (rng() & 0xff);
                for (size_t b = 0; b < (size_t) N * nb; ++b) {
                    const uint16_t dh = wa_q1_f2h(b % 7 == 0 ? 3e-6f * uni(rng) : 0.02f * uni(rng)), mh = wa_q1_f2h(b % 5 == 0 ? 0.0f : 0.01f * uni(rng));
                    memcpy(&raw[b * bsz], &dh, 2);
                    if (k) memcpy(&raw[b * bsz + 2], &mh, 2);
                }
                for (int M : { 1, 3, 4, 5, 7, 8, 21 }) {          // (21: the gemm's 16-row loop, a group of four behind it, one leftover row)
                    std::vector<float> x((size_t) M * K);
                    for (size_t i = 0; i < x.size(); ++i) x[i] = gauss(rng) * powf(10.0f, -2.0f + (float) ((i / per) % 5));
                    for (int m : { 0, M - 1 }) {
                        float * xb = &x[(size_t) m * K];
                        for (int e = 0; e < per; ++e) xb[e] = (float) (e % 20) + 0.5f;          // |scale| = 1: every product at a tie of rint
                        xb[5] = -127.0f; xb[21] = 127.0f;                                        // - m before + m
                        if (nb >= 3) for (int e = 0; e < per; ++e) xb[per + e] = 0.0f;           // an all-zero block
                    }
                    check(k, blk, N, K, x, M, "dot");
                    check(k, raw, N, K, x, M, "dot (raw blocks)");
                }
            }
    printf("quant4: %ld values checked\n", n_checked);
    printf("quant4: %ld mismatches\n", n_bad);
    return n_bad == 0 ? 0 : 1;
}

// quantw_math - wa_quantw.h against the reference library's ggml_quantize_chunk, byte for byte (tests/test_quantw_math.py).
//   quantw_math <libwhisper_ref.so> <type> <rows.f32> <rows.f16>
// rows.f32: F32 values, rows.f16: IEEE halfs; both a multiple of 256 long.  One line per source: "quantw: type T src S blocks N bad B".
#include "wa_quantw.h"

#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include <vector>

struct init_params { size_t mem_size; void * mem_buffer; bool no_alloc; };        // ggml_init_params
typedef size_t (*quantize_chunk_fn)(int type, const float * src, void * dst, int64_t start, int64_t nrows, int64_t n_per_row, const float * imatrix);

static std::vector<uint8_t> slurp(const char * path) {
    std::vector<uint8_t> v;
    FILE * f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + n);
    fclose(f);
    return v;
}

int main(int argc, char ** argv) {
    if (argc != 5) return 2;
    void * lib = dlopen(argv[1], RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    quantize_chunk_fn ref = (quantize_chunk_fn) dlsym(lib, "ggml_quantize_chunk");
    if (!ref) { fprintf(stderr, "no ggml_quantize_chunk\n"); return 2; }
    // the reference's F16 -> F32 table is filled by ggml_init (its quantize tool calls it first for that reason): without it every d reads as 0
    void * (*init)(init_params) = (void * (*)(init_params)) dlsym(lib, "ggml_init");
    if (!init || !init(init_params{ 1 << 20, nullptr, false })) { fprintf(stderr, "ggml_init failed\n"); return 2; }
    if (void (*cpu_init)(void) = (void (*)(void)) dlsym(lib, "ggml_cpu_init")) cpu_init();
    const int type = atoi(argv[2]);
    const std::vector<uint8_t> f32 = slurp(argv[3]), f16 = slurp(argv[4]);
    const size_t bv = (size_t) wa_qw_block_values(type), bs = wa_qw_block_bytes(type);
    if (!bv) return 2;
    int rc = 0;
    for (int src = 0; src < 2; ++src) {
        const int64_t n = (int64_t) (src == 0 ? f32.size() / 4 : f16.size() / 2);
        std::vector<float> x((size_t) n);
        if (src == 0) memcpy(x.data(), f32.data(), (size_t) n * 4);
        else for (int64_t i = 0; i < n; ++i) { uint16_t h; memcpy(&h, f16.data() + 2 * i, 2); x[(size_t) i] = wa_q1_h2f(h); }
        std::vector<uint8_t> want((size_t) n / bv * bs, 0xa5), got(want.size(), 0x5a);
        if (ref(type, x.data(), want.data(), 0, 1, n, nullptr) != want.size()) { printf("quantw: reference size differs\n"); return 1; }
        const int e = src == 0 ? wa_quantw_rows(type, x.data(), n, got.data()) : wa_quantw_rows_f16(type, (const uint16_t *) f16.data(), n, got.data());
        if (e) { printf("quantw: wa_quantw_rows returned %d\n", e); return 1; }
        size_t bad = 0;
        for (size_t b = 0; b < (size_t) n / bv; ++b)
            if (memcmp(want.data() + b * bs, got.data() + b * bs, bs) != 0) { if (!bad) printf("quantw: type %d src %d first bad block %zu\n", type, src, b); ++bad; }
        printf("quantw: type %d src %d blocks %zu bad %zu\n", type, src, (size_t) n / bv, bad);
        if (bad) rc = 1;
    }
    // the refusals: another type, a ragged length, a value that is not finite
    std::vector<float> x(256, 1.0f); std::vector<uint8_t> y(1024);
    const int r1 = wa_quantw_rows(10, x.data(), 256, y.data()), r2 = wa_quantw_rows(type, x.data(), 16, y.data());
    x[200] = INFINITY;
    const int r3 = wa_quantw_rows(type, x.data(), 256, y.data());
    printf("quantw: refusals %d %d %d\n", r1, r2, r3);
    return rc;
}

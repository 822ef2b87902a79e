// dtw_math.cpp - driver of the DTW host arithmetic (whisper-rust_amd/csrc/wa_dtw_host.cpp, compiled alone by g++: no HIP, no device) for
// tests/test_dtw_math.py.
//
//   dtw_math <in> <out>
// in:  int32 n_cases, then per case int32 { n_heads, n_tokens, n_ctx, M, sot_len, medfilt_width } and the cube f32 [n_heads][n_tokens][n_ctx]
// out: per case int32 rc (the path length, or the refusal), and when rc >= 0: int32 n_cost, cost_in f32 [n_tokens][M], the path as
//      int32 pairs (token index, time index)
// The cube is read through a view with the heads in reverse order in memory and a token stride larger than n_ctx, as the capture buffer has.
#include "wa_dtw_host.h"

#include <cstdio>
#include <cstdlib>

static bool rd(FILE * f, void * p, size_t n) { return fread(p, 1, n, f) == n; }

int main(int argc, char ** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s in out\n", argv[0]); return 2; }
    FILE * fi = fopen(argv[1], "rb"), * fo = fopen(argv[2], "wb");
    if (!fi || !fo) { fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t n_cases = 0;
    if (!rd(fi, &n_cases, 4)) return 2;
    for (int c = 0; c < n_cases; ++c) {
        int32_t h[6];
        if (!rd(fi, h, sizeof(h))) return 2;
        const int n_heads = h[0], n_tokens = h[1], n_ctx = h[2], M = h[3], sot_len = h[4], width = h[5];
        if (n_heads <= 0 || n_tokens <= 0 || n_ctx <= 0 || n_heads > 64 || n_tokens > 4096 || n_ctx > 4096) return 2;
        std::vector<float> cube((size_t) n_heads * n_tokens * n_ctx);
        if (!rd(fi, cube.data(), cube.size() * 4)) return 2;
        // strided copy: head k at slot n_heads - 1 - k, rows padded by 5 floats
        const long long ts = n_ctx + 5;
        std::vector<float> buf((size_t) n_heads * n_tokens * ts, -7.0f);
        std::vector<long long> off(n_heads);
        for (int k = 0; k < n_heads; ++k) {
            off[k] = (long long) (n_heads - 1 - k) * n_tokens * ts;
            for (int t = 0; t < n_tokens; ++t)
                for (int j = 0; j < n_ctx; ++j) buf[off[k] + t * ts + j] = cube[((size_t) k * n_tokens + t) * n_ctx + j];
        }
        const wa_dtw_view v = { buf.data(), off.data(), n_heads, ts, n_tokens, n_ctx };
        wa_dtw_path_t path;
        std::vector<float> cost;
        const int32_t rc = wa_dtw_host_path(v, M, sot_len, width, path, &cost);
        fwrite(&rc, 4, 1, fo);
        if (rc < 0) continue;
        const int32_t n_cost = (int32_t) cost.size();
        fwrite(&n_cost, 4, 1, fo);
        fwrite(cost.data(), 4, cost.size(), fo);
        for (const auto & p : path) { const int32_t pr[2] = { p.first, p.second }; fwrite(pr, 4, 2, fo); }
    }
    fclose(fi);
    if (fclose(fo) != 0) return 2;
    return 0;
}

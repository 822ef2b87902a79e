// Kernel-level harness of the Q4_0 / Q4_K paths (tests/test_quant4_kernels_gpu.py): C entry points around the product's own launchers (wa_load.hip, wa_quant4.hip, the
// plain-order kernels and quantisers of wa_quant.hip / wa_quantk.hip; linked against the product's objects, not a recompile) and the host statement they are held to
// (wa_quant4.h).  k != 0: Q4_K, else Q4_0.  Every call allocates, runs, copies back, frees and returns a hipError_t as an int.
#include "wa_kernels.h"
#include "wa_load.h"
#include "wa_quant4.h"

#include <vector>

#define CK(x) do { const hipError_t q4_e = (x); if (q4_e != hipSuccess) return (int) q4_e; } while (0)
#define UP(buf, host, count) do { if (int q4_r = (buf).up((host), (count))) return q4_r; } while (0)
#define DOWN(buf, host) do { if (int q4_r = (buf).down(host)) return q4_r; } while (0)

template <class T> struct dbuf {        // a device copy of a host array (null host pointer: no buffer)
    T * p = nullptr; size_t n = 0;
    int up(const T * h, size_t count) { n = count; if (!h || !count) return 0; CK(hipMalloc(&p, n * sizeof(T))); CK(hipMemcpy(p, h, n * sizeof(T), hipMemcpyHostToDevice)); return 0; }
    int down(T * h) { if (p) CK(hipMemcpy(h, p, n * sizeof(T), hipMemcpyDeviceToHost)); return 0; }
    ~dbuf() { if (p) (void) hipFree(p); }
};
struct q4k_epi {        // the fields of wa_epi a test sets; the out arrays are the caller's, pre-filled, and come back as the kernel left them
    const float * bias, * scale, * resid; const uint16_t * gelu;
    int split0, split1, row_off, aux0, aux1, ldo, ldo2, ldo3, ldr;
    uint8_t * out, * out2, * out3; size_t out_bytes, out2_bytes, out3_bytes;
};
struct q4k_x { dbuf<float> x, d; dbuf<int8_t> q; dbuf<int16_t> bs; };      // activation rows on the device: F32 and quantised (zero-filled until a kernel writes them)
static int x_up(q4k_x & a, const float * x, int M, int K) {
    std::vector<int8_t> z((size_t) M * K); std::vector<float> zf((size_t) M * K / 32); std::vector<int16_t> zs((size_t) M * K / 16);
    UP(a.x, x, (size_t) M * K); UP(a.q, z.data(), z.size()); UP(a.d, zf.data(), zf.size()); UP(a.bs, zs.data(), zs.size());
    return 0;
}

// x f32 [M][K] -> Q8_K rows in the kernel layout: rule 0 wa_launch_quantize_q8_K (the row rule), 1 wa_launch_quantize_q8_K4 (rows below M - M % 4 by the four-row rule)
extern "C" int q4k_quant(int rule, int M, int K, const float * x, int8_t * qs, float * qd, int16_t * qbs) {
    q4k_x a;
    if (int r = x_up(a, x, M, K)) return r;
    (rule ? wa_launch_quantize_q8_K4 : wa_launch_quantize_q8_K)(nullptr, a.x.p, K, M, K, a.q.p, a.d.p, a.bs.p);
    CK(hipDeviceSynchronize());
    a.d.n = (size_t) M * K / 256;
    DOWN(a.q, qs); DOWN(a.d, qd); DOWN(a.bs, qbs);
    return 0;
}
extern "C" void q4k_host_quant(int rule, int M, int K, const float * x, int8_t * qs, float * qd, int16_t * qbs) {      // the same rows by the host statement
    const int nb = K / 256;
    std::vector<int8_t> q(K);
    for (int m = 0; m < M; ++m) {
        (rule && m < wa_q4_K_rows4(M) ? wa_q8_K_row4 : wa_q8_K_row)(x + (size_t) m * K, nb, q.data(), qd + (size_t) m * nb, qbs + (size_t) m * nb * 16);
        for (int i = 0; i < K; ++i) qs[wa_qk_quant_index(m, nb, i >> 8, i & 255)] = q[i];
    }
}

// raw blocks [N][..] -> the arena arrays by the device load kernel (returned: qs N K / 2 bytes, qd; Q4_K: qsc, qm too), x -> activation rows by the product's quantiser,
// then the interleaved product with the route and the epilogue given
extern "C" int q4k_gemm(int k, int mode, int route, int M, int N, int K, const float * x, const uint8_t * blk, const q4k_epi * ep, uint8_t * qs, uint8_t * qsc, float * qd, float * qm) {
    const size_t nb = (size_t) K / (k ? 256 : 32);
    dbuf<uint8_t> dblk, dq, dsc, o1, o2, o3; dbuf<float> dd, dm, bias, scale, resid; dbuf<uint16_t> gelu; q4k_x a;
    UP(dblk, blk, N * nb * (k ? WA_Q4_K_BYTES : WA_Q4_0_BYTES)); UP(dq, qs, (size_t) N * K / 2); UP(dsc, qsc, N * nb * 16); UP(dd, qd, N * nb); UP(dm, qm, N * nb);
    if (int r = x_up(a, x, M, K)) return r;
    UP(bias, ep->bias, N); UP(scale, ep->scale, N); UP(resid, ep->resid, (size_t) M * ep->ldr); UP(gelu, ep->gelu, 65536);
    UP(o1, ep->out, ep->out_bytes); UP(o2, ep->out2, ep->out2_bytes); UP(o3, ep->out3, ep->out3_bytes);
    wa_epi e;
    e.bias = bias.p; e.scale = scale.p; e.resid = resid.p; e.ldr = ep->ldr; e.gelu = gelu.p;
    e.out = o1.p; e.ldo = ep->ldo; e.out2 = o2.p; e.ldo2 = ep->ldo2; e.out3 = o3.p; e.ldo3 = ep->ldo3;
    e.split0 = ep->split0; e.split1 = ep->split1; e.row_off = ep->row_off; e.aux0 = ep->aux0; e.aux1 = ep->aux1;
    if (k) {
        CK((hipError_t) wa_launch_load_q4_K(nullptr, dblk.p, N, nb, 0, dq.p, (int8_t *) dsc.p, dd.p, dm.p));
        wa_launch_quantize_q8_K4(nullptr, a.x.p, K, M, K, a.q.p, a.d.p, a.bs.p);
        wa_launch_q4kgemm_route(nullptr, (wa_epi_mode) mode, a.q.p, a.d.p, a.bs.p, M, dq.p, dsc.p, dd.p, dm.p, N, K, e, route);
    } else {
        CK((hipError_t) wa_launch_load_q4_0(nullptr, dblk.p, N, nb, 0, dq.p, dd.p));
        wa_launch_quantize_q8_0(nullptr, a.x.p, K, M, K, a.q.p, a.d.p);
        wa_launch_q4gemm_route(nullptr, (wa_epi_mode) mode, a.q.p, a.d.p, M, dq.p, dd.p, N, K, e, route);
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    DOWN(dq, qs); DOWN(dsc, qsc); DOWN(dd, qd); DOWN(dm, qm); DOWN(o1, ep->out); DOWN(o2, ep->out2); DOWN(o3, ep->out3);
    return 0;
}
extern "C" int q4k_kernel(int M, int route) { return wa_q4gemm_kernel(M, route); }

// the plain matrix (the token embedding): device load, the logits product out [M][N], and the embedding fetch emb [n_tok][K] = row tok[j] + pe[pos[j]]
extern "C" int q4k_plain(int k, int M, int N, int K, const float * x, const uint8_t * blk, float * out, int n_tok, const int32_t * tok, const int32_t * pos, const float * pe, int n_pos, float * emb) {
    const size_t nb = (size_t) K / (k ? 256 : 32);
    dbuf<uint8_t> dblk; dbuf<float> dd, dm, dout, dpe, demb; dbuf<int8_t> dq, dsc; dbuf<int32_t> dtok, dpos; q4k_x a;
    std::vector<int8_t> z((size_t) N * K); std::vector<float> zf(N * nb);
    UP(dblk, blk, N * nb * (k ? WA_Q4_K_BYTES : WA_Q4_0_BYTES)); UP(dq, z.data(), z.size()); UP(dsc, z.data(), N * nb * 16); UP(dd, zf.data(), zf.size()); UP(dm, zf.data(), zf.size());
    if (int r = x_up(a, x, M, K)) return r;
    UP(dout, out, (size_t) M * N); UP(dtok, tok, n_tok); UP(dpos, pos, n_tok); UP(dpe, pe, (size_t) n_pos * K); UP(demb, emb, (size_t) n_tok * K);
    if (k) {
        CK((hipError_t) wa_launch_load_q4_K(nullptr, dblk.p, N, nb, 1, dq.p, dsc.p, dd.p, dm.p));
        wa_launch_quantize_q8_K(nullptr, a.x.p, K, M, K, a.q.p, a.d.p, a.bs.p);
        wa_launch_q4k_plain(nullptr, a.q.p, a.d.p, a.bs.p, M, dq.p, dsc.p, dd.p, dm.p, N, K, dout.p, N);
        wa_launch_dec_embed_k(nullptr, WA_TYPE_Q5_K, dtok.p, dpos.p, n_tok, K, dq.p, dsc.p, dd.p, dm.p, dpe.p, demb.p);
    } else {
        CK((hipError_t) wa_launch_load_q4_0(nullptr, dblk.p, N, nb, 1, dq.p, dd.p));
        wa_launch_quantize_q8_0(nullptr, a.x.p, K, M, K, a.q.p, a.d.p);
        wa_epi e; e.out = dout.p; e.ldo = N;
        wa_launch_qgemm_exact(nullptr, WA_EPI_F32, a.q.p, a.d.p, M, dq.p, dd.p, N, K, e);
        wa_launch_dec_embed_q(nullptr, dtok.p, dpos.p, n_tok, K, dq.p, dd.p, dpe.p, demb.p);
    }
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    DOWN(dout, out); DOWN(demb, emb);
    return 0;
}

// ---- the host statement ----
extern "C" void q4k_host_pack(int k, const uint8_t * blk, int N, int K, uint8_t * qs, uint8_t * qsc, float * qd, float * qm) {
    if (k) wa_q4_K_pack_rows(blk, N, K / 256, qs, qsc, qd, qm); else wa_q4_0_pack_rows(blk, N, K / 32, qs, qd);
}
// acc [M][N] of the interleaved (plain == 0: Q4_K's quantiser and chain steps by the row's place in M) or the plain product; deq [N][K] the dequantised matrix
extern "C" void q4k_host_dot(int k, int plain, int M, int N, int K, const float * x, const uint8_t * blk, float * acc, float * deq) {
    const int nb = K / (k ? 256 : 32), n4 = k && !plain ? wa_q4_K_rows4(M) : 0;
    std::vector<int8_t> xq((size_t) M * K), wq(K); std::vector<float> xd((size_t) M * nb), wd(nb), wdm(nb); std::vector<int16_t> xbs((size_t) M * K / 16); std::vector<uint8_t> wsc(K / 16);
    for (int m = 0; m < M; ++m)
        if (k) (m < n4 ? wa_q8_K_row4 : wa_q8_K_row)(x + (size_t) m * K, nb, &xq[(size_t) m * K], &xd[(size_t) m * nb], &xbs[(size_t) m * nb * 16]);
        else wa_q8_0_row(x + (size_t) m * K, nb, &xq[(size_t) m * K], &xd[(size_t) m * nb]);
    for (int n = 0; n < N; ++n) {
        for (int b = 0; b < nb; ++b)
            if (k) wa_q4_K_unpack(blk + ((size_t) n * nb + b) * WA_Q4_K_BYTES, &wq[256 * b], &wsc[16 * b], wd[b], wdm[b]); else wa_q4_0_unpack(blk + ((size_t) n * nb + b) * WA_Q4_0_BYTES, &wq[32 * b], wd[b]);
        for (int i = 0; i < K; ++i)
            deq[(size_t) n * K + i] = k ? wa_qk_dequant(WA_TYPE_Q5_K, &wq[i & ~255], (const int8_t *) &wsc[16 * (i >> 8)], wd[i >> 8], wdm[i >> 8], i & 255) : wa_q4_0_dequant(wq[i], wd[i >> 5]);
        for (int m = 0; m < M; ++m) {
            const int8_t * q = &xq[(size_t) m * K]; const float * d = &xd[(size_t) m * nb]; const int16_t * bs = &xbs[(size_t) m * nb * (k ? 16 : 0)];
            acc[(size_t) m * N + n] = k ? (plain ? wa_q4_K_dot_plain(nb, wq.data(), wsc.data(), wd.data(), wdm.data(), q, d, bs) : wa_q4_K_dot8(nb, wq.data(), wsc.data(), wd.data(), wdm.data(), q, d, bs, m < n4))
                                        : (plain ? wa_q4_0_dot_plain(nb, wq.data(), wd.data(), q, d) : wa_q4_0_dot8(nb, wq.data(), wd.data(), q, d));
        }
    }
}

// stream_vad_kernels.hip - TEST INFRASTRUCTURE ONLY: C entry points around the launcher of k_stream_vad_front (wa_vad.hip), the VAD front end
// on ring windows of several live sessions, for tests/test_stream_vad_kernels_gpu.py.  Linked against the product's own
// whisper-rust_amd/build/wa_vad_k.o (whisper-rust_amd/Makefile, target `stream_vad_harness`), so the kernel under test is the one
// libwhisper.so ships (wa_stream_k.o beside it: tools/stream_vad_probe.py times the new launch against the gather and front-end launches
// that existed before).  The tests' launches go to the null stream.
#include "wa_stream.h"
#include "wa_vad.h"

#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstring>

#define SV_API extern "C" __attribute__((visibility("default")))
#define SV_GUARD 64         // NaN floats on both sides of every ring and of every session's output rows

static void * g_weights = nullptr;
static wa_vad_dev g_dev;

SV_API int svtest_sessions(void) { return WA_SVAD_SESSIONS; }
SV_API int svtest_max_windows(void) { return WA_SVAD_MAX_WINDOWS; }

// The model's tensors as the file holds them (F16 as uint16): uploaded in the layout the product uses - one allocation, every tensor on a
// 256-byte boundary, layer 0's rows padded from 387 to WA_VAD_LD0 halfs.  Returns 0, -2 a HIP call failed.
SV_API int svtest_set_weights(const uint16_t * stft, const uint16_t * w0, const uint16_t * w1, const uint16_t * w2, const uint16_t * w3, const float * b0,
                              const float * b1, const float * b2, const float * b3, const float * w_ih, const float * b_ih) {
    std::vector<uint8_t> img;
    auto put = [&](const void * src, size_t bytes) { const size_t at = (img.size() + 255) & ~(size_t) 255; img.resize(at + bytes); memcpy(img.data() + at, src, bytes); return at; };
    std::vector<uint16_t> p0((size_t) 128 * WA_VAD_LD0, 0);
    for (int r = 0; r < 128; ++r) memcpy(&p0[(size_t) r * WA_VAD_LD0], w0 + (size_t) r * 387, 387 * sizeof(uint16_t));
    const uint16_t * w[4] = { p0.data(), w1, w2, w3 };
    const float * b[4] = { b0, b1, b2, b3 };
    const size_t wn[4] = { p0.size(), (size_t) 64 * 384, (size_t) 64 * 192, (size_t) 128 * 192 }, bn[4] = { 128, 64, 64, 128 };
    size_t o_w[4], o_b[4];
    const size_t o_stft = put(stft, (size_t) 258 * 256 * 2);
    for (int i = 0; i < 4; ++i) o_w[i] = put(w[i], wn[i] * 2);
    for (int i = 0; i < 4; ++i) o_b[i] = put(b[i], bn[i] * 4);
    const size_t o_wih = put(w_ih, (size_t) 512 * 128 * 4), o_bih = put(b_ih, (size_t) 512 * 4);
    img.resize(img.size() + 256);
    if (g_weights) { (void) hipFree(g_weights); g_weights = nullptr; }
    if (hipMalloc(&g_weights, img.size()) != hipSuccess || hipMemcpy(g_weights, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) return -2;
    const uint8_t * base = (const uint8_t *) g_weights;
    g_dev.stft = (const uint16_t *) (base + o_stft);
    for (int i = 0; i < 4; ++i) { g_dev.enc_w[i] = (const uint16_t *) (base + o_w[i]); g_dev.enc_b[i] = (const float *) (base + o_b[i]); }
    g_dev.w_ih = (const float *) (base + o_wih);
    g_dev.b_ih = (const float *) (base + o_bih);
    return 0;
}

// For tools/stream_vad_probe.py: the front end of one poll - n_windows new windows in each of n_sessions (<= 8) rings of `cap` samples, the
// windows wrapping at the ring's end - timed from the first launch to the host seeing the gate inputs, `iters` times after 5 unmeasured ones.
// mode 0: ONE k_stream_vad_front launch that writes the sessions' pinned buffers, one stream synchronise.  mode 1, the same work with the
// pieces that existed before: per session one k_stream_window gather into a staging buffer, one k_vad_front launch on it, one copy of its
// result to the pinned buffer; one stream synchronise at the end.  us[i] receives iteration i's wall time in microseconds.
// Returns 0, -1 refused arguments, -2 a HIP call failed, -3 a launcher refused.
SV_API int svtest_time(int mode, int n_sessions, int n_windows, int cap, int iters, double * us) {
    if (!g_weights || n_sessions <= 0 || n_sessions > WA_SVAD_SESSIONS || n_windows <= 0 || n_windows * WA_VAD_WINDOW > cap || iters <= 0) return -1;
    const size_t nw = (size_t) n_windows, ring_f = (size_t) cap + 4;
    float * d_rings = nullptr, * d_stage = nullptr, * d_gates = nullptr, * h_out = nullptr;
    hipStream_t q = nullptr;
    int ret = -2;
    do {
        if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess) break;
        if (hipMalloc((void **) &d_rings, n_sessions * ring_f * sizeof(float)) != hipSuccess || hipMemset(d_rings, 0, n_sessions * ring_f * sizeof(float)) != hipSuccess) break;
        if (hipMalloc((void **) &d_stage, n_sessions * nw * WA_VAD_WINDOW * sizeof(float)) != hipSuccess) break;
        if (hipMalloc((void **) &d_gates, n_sessions * nw * WA_VAD_GATES * sizeof(float)) != hipSuccess) break;
        if (hipHostMalloc((void **) &h_out, n_sessions * nw * WA_VAD_GATES * sizeof(float), hipHostMallocDefault) != hipSuccess) break;
        const int slot = cap - 300;                 // the first window wraps
        wa_svad_table tab;
        memset(&tab, 0, sizeof(tab));
        wa_stream_windows win;
        memset(&win, 0, sizeof(win));
        for (int i = 0; i < n_sessions; ++i) {
            tab.s[i].ring = d_rings + i * ring_f; tab.s[i].out = h_out + i * nw * WA_VAD_GATES;
            tab.s[i].cap = cap; tab.s[i].slot = slot; tab.s[i].n_valid = n_windows * WA_VAD_WINDOW;
            tab.first[i + 1] = tab.first[i] + n_windows;
        }
        tab.n_sessions = n_sessions;
        bool ok = true;
        for (int it = -5; it < iters && ok; ++it) {
            const auto t0 = std::chrono::steady_clock::now();
            if (mode == 0) ok = wa_svad_front_launch(g_dev, tab, (void *) q);
            else for (int i = 0; i < n_sessions && ok; ++i) {
                wa_stream_window & w = win.w[0];
                w.ring = d_rings + i * ring_f; w.dst = d_stage + i * nw * WA_VAD_WINDOW; w.len = n_windows * WA_VAD_WINDOW;
                w.n_pieces = wa_stream_ring_pieces(slot, w.len, cap, w.slot, w.plen);
                float * g = d_gates + i * nw * WA_VAD_GATES;
                ok = wa_stream_window_launch((void *) q, win, 1) && wa_vad_front_launch(g_dev, w.dst, w.len, n_windows, g, (void *) q) &&
                     hipMemcpyAsync(h_out + i * nw * WA_VAD_GATES, g, nw * WA_VAD_GATES * sizeof(float), hipMemcpyDeviceToHost, q) == hipSuccess;
            }
            if (!ok) { ret = -3; break; }
            if (hipStreamSynchronize(q) != hipSuccess) { ok = false; ret = -2; break; }
            if (it >= 0) us[it] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        }
        if (ok) ret = 0;
    } while (false);
    if (q) { (void) hipStreamSynchronize(q); (void) hipStreamDestroy(q); }
    if (d_rings) (void) hipFree(d_rings);
    if (d_stage) (void) hipFree(d_stage);
    if (d_gates) (void) hipFree(d_gates);
    if (h_out) (void) hipHostFree(h_out);
    return ret;
}

// ONE launch of k_stream_vad_front over n_sessions (<= 8) sessions.  Session i owns a ring of cap[i] floats that starts ring_off[i] floats
// (0 .. 3) behind a 16-byte boundary, NaN everywhere - guards of SV_GUARD floats on both sides and every slot - except where its n_samples[i]
// samples (taken from `samples`, the sessions' samples one after another) lie: sample q in slot (slot[i] + q) mod cap[i].  It asks for
// n_windows[i] windows (0 allowed), the last one partial where n_samples[i] is no multiple of 512.  `out` receives, per session, `row` floats
// of a PINNED buffer the kernel wrote: [guard][n_windows[i] x 512 gate inputs][NaN to the end]; everything was NaN before the launch.
// After the launch the guarded rings are read back and compared with what was uploaded, bit for bit.
// Returns 0, -1 refused arguments, -2 a HIP call failed, -3 the launcher refused, -4 the launch changed a ring or its guards.
SV_API int svtest_run(int n_sessions, const float * samples, const int * n_samples, const int * n_windows, const int * cap, const int * slot,
                      const int * ring_off, float * out, long long row) {
    if (!g_weights || n_sessions <= 0 || n_sessions > WA_SVAD_SESSIONS || row <= 0) return -1;
    const long long G = SV_GUARD;
    const float nan = std::nanf("");
    wa_svad_table tab;
    memset(&tab, 0, sizeof(tab));
    long long ring_total = 0;
    for (int i = 0; i < n_sessions; ++i) {
        if (cap[i] <= 0 || slot[i] < 0 || slot[i] >= cap[i] || ring_off[i] < 0 || ring_off[i] > 3 || n_windows[i] < 0 || n_samples[i] < 0 || n_samples[i] > cap[i]) return -1;
        if (n_windows[i] > 0 && (n_samples[i] <= (n_windows[i] - 1) * WA_VAD_WINDOW || n_samples[i] > n_windows[i] * WA_VAD_WINDOW)) return -1;
        if (n_windows[i] == 0 && n_samples[i] != 0) return -1;
        if (2 * G + (long long) n_windows[i] * WA_VAD_GATES > row) return -1;
        ring_total += 2 * G + 4 + (cap[i] + 3) / 4 * 4;
    }
    std::vector<float> rings((size_t) ring_total, nan);
    std::vector<long long> at((size_t) n_sessions);
    {
        long long o = 0, q0 = 0;
        for (int i = 0; i < n_sessions; ++i) {
            at[(size_t) i] = o + G + ring_off[i];
            for (int q = 0; q < n_samples[i]; ++q) rings[(size_t) (at[(size_t) i] + (slot[i] + q) % cap[i])] = samples[q0 + q];
            q0 += n_samples[i];
            o += 2 * G + 4 + (cap[i] + 3) / 4 * 4;
        }
    }
    float * d_rings = nullptr, * h_out = nullptr;
    int ret = -2;
    do {
        if (hipMalloc((void **) &d_rings, rings.size() * sizeof(float)) != hipSuccess) break;
        if (hipHostMalloc((void **) &h_out, (size_t) n_sessions * row * sizeof(float), hipHostMallocDefault) != hipSuccess) break;
        if (hipMemcpy(d_rings, rings.data(), rings.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) break;
        for (long long k = 0; k < n_sessions * row; ++k) h_out[k] = nan;
        for (int i = 0; i < n_sessions; ++i) {
            tab.s[i].ring = d_rings + at[(size_t) i];
            tab.s[i].out = h_out + (size_t) i * row + G;
            tab.s[i].cap = cap[i]; tab.s[i].slot = slot[i]; tab.s[i].n_valid = n_samples[i];
            tab.first[i + 1] = tab.first[i] + n_windows[i];
        }
        tab.n_sessions = n_sessions;
        if (!wa_svad_front_launch(g_dev, tab, nullptr)) { ret = -3; break; }
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) break;
        memcpy(out, h_out, (size_t) n_sessions * row * sizeof(float));
        std::vector<float> after(rings.size());
        if (hipMemcpy(after.data(), d_rings, rings.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) break;
        ret = memcmp(after.data(), rings.data(), rings.size() * sizeof(float)) == 0 ? 0 : -4;
    } while (false);
    if (d_rings) (void) hipFree(d_rings);
    if (h_out) (void) hipHostFree(h_out);
    return ret;
}

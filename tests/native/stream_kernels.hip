// stream_kernels.hip - TEST INFRASTRUCTURE ONLY: C entry points around the launchers of wa_stream.hip (the streaming sessions' kernels) and
// around the host restatement of wa_stream.h they are held to, for tests/test_stream_kernels_gpu.py.  Linked against the product's own
// whisper-rust_amd/build/wa_stream_k.o (whisper-rust_amd/Makefile, target `stream_harness`), so the kernels under test are the ones
// libwhisper.so ships.  Launches go to the null stream.
#include "wa_stream.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#define ST_API extern "C" __attribute__((visibility("default")))
#define ST_GUARD 64         // NaN floats on both sides of the ring, of each carry buffer and of each window destination

ST_API int stest_tile(void) { return WA_STREAM_TILE; }
ST_API long long stest_final(int rate, long long T) { wa_audio_plan p; return wa_audio_plan_make(rate, p) ? wa_stream_final(p, T) : -1; }
ST_API int stest_carry_len(int rate) { wa_audio_plan p; return wa_audio_plan_make(rate, p) ? wa_stream_carry_len(p) : -1; }
// floats of one image: [guard][ring: cap][guard][carry: C][guard][other carry: C][guard]
ST_API long long stest_image_len(int rate, long long cap) { const int C = stest_carry_len(rate); return C < 0 ? -1 : cap + 2 * (long long) C + 4 * ST_GUARD; }

// A recording fed in `packets` (frame counts that sum to n_frames) and flushed, where = 0 through wa_stream_ref, where = 1 through
// k_stream_push on a device copy of the recording (every packet read where it lies in that copy: its alignment is whatever the split gives).
// The ring holds `cap` samples.  An IMAGE - the guarded ring, then the guarded carry, then the guarded other carry buffer - is written to
// `images` whenever the next push would overwrite a sample written since the last image, and once at the end: every output appears in one.
// The carry comes first of the two where it is the session's current one.  Returns the number of images, or -1 refused arguments,
// -2 a HIP call failed, -3 the launcher refused, -5 more than max_images.
ST_API long long stest_push_run(int rate, int format, int channels, const void * data, long long n_frames, const long long * packets, int n_packets,
                                long long cap, int where, float * images, int max_images) {
    wa_stream_ref R;
    if (!wa_audio_args_ok(data, n_frames, channels, rate, format) || cap <= 0 || !R.init(rate, channels, format, cap)) return -1;
    const wa_audio_plan p = R.ap;
    const long long C = wa_stream_carry_len(p), Z = wa_stream_flush_frames(p), G = ST_GUARD, img = stest_image_len(rate, cap);
    const size_t fb = (size_t) channels * (format == WA_AUDIO_I16 ? 2 : 4);
    const float nan = std::nanf("");
    std::vector<float> host((size_t) img, nan), made;
    uint8_t * d_in = nullptr, * d_zero = nullptr;
    float * d_img = nullptr, * d_taps = nullptr;
    long long ret = -2, n_images = 0;
    do {
        float * d_ring = nullptr, * d_carry[2] = { nullptr, nullptr };
        if (where == 1) {
            if (hipMalloc((void **) &d_in, (size_t) n_frames * fb + 256) != hipSuccess || hipMalloc((void **) &d_img, (size_t) img * sizeof(float)) != hipSuccess ||
                hipMalloc((void **) &d_zero, (size_t) (Z + 1) * fb) != hipSuccess) break;
            if (hipMemcpy(d_in, data, (size_t) n_frames * fb, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_zero, 0, (size_t) (Z + 1) * fb) != hipSuccess) break;
            for (long long i = 0; i < cap; ++i) host[(size_t) (G + i)] = 0.0f;
            for (long long i = 0; i < C; ++i) host[(size_t) (2 * G + cap + i)] = host[(size_t) (3 * G + cap + C + i)] = 0.0f;
            if (hipMemcpy(d_img, host.data(), (size_t) img * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) break;
            d_ring = d_img + G; d_carry[0] = d_img + 2 * G + cap; d_carry[1] = d_img + 3 * G + cap + C;
            if (p.K) {
                if (hipMalloc((void **) &d_taps, R.taps.size() * sizeof(float)) != hipSuccess) break;
                if (hipMemcpy(d_taps, R.taps.data(), R.taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) break;
            }
        }
        long long T = 0, n_out = 0, r_w = 0, since = 0;
        int cur = 0;
        bool bad = false;
        auto image = [&]() {
            if (n_images >= max_images) { ret = -5; return false; }
            float * dst = images + (size_t) n_images * (size_t) img;
            if (where == 1) {
                if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(host.data(), d_img, (size_t) img * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return false;
                memcpy(dst, host.data(), (size_t) (2 * G + cap) * sizeof(float));
                const float * a = host.data() + 2 * G + cap, * b = a + G + C;       // each [carry][guard]; the current one first
                memcpy(dst + 2 * G + cap, cur == 0 ? a : b, (size_t) (C + G) * sizeof(float));
                memcpy(dst + 3 * G + cap + C, cur == 0 ? b : a, (size_t) (C + G) * sizeof(float));
            } else {
                for (long long i = 0; i < img; ++i) dst[i] = nan;
                memcpy(dst + G, R.ring.data(), (size_t) cap * sizeof(float));
                if (C) memcpy(dst + 2 * G + cap, R.carry.data(), (size_t) C * sizeof(float));
            }
            ++n_images; since = 0;
            return true;
        };
        for (int k = 0; k <= n_packets && !bad; ++k) {          // the last round is the flush
            const bool flush = k == n_packets;
            const long long F = flush ? Z : packets[k];
            if (F < 0 || (!flush && T + F > n_frames)) { ret = -1; bad = true; break; }
            if (F == 0) continue;
            const long long n_new = wa_stream_final(p, T + F) - n_out;
            if (n_new > cap) { ret = -1; bad = true; break; }
            if (since + n_new > cap && !image()) { bad = true; break; }
            if (where == 1) {
                const void * src = flush ? (const void *) d_zero : (const void *) (d_in + (size_t) T * fb);
                if (!wa_stream_push_launch(nullptr, src, F, channels, format, p, d_taps, T, d_carry[cur], d_carry[cur ^ 1], n_out, n_new, d_ring, cap, r_w)) {
                    ret = -3; bad = true; break;
                }
                if (p.K) cur ^= 1;
            } else {
                made.assign((size_t) std::max<long long>(n_new, 1), 0.0f);
                R.T = T; R.n_out = n_out;
                const std::vector<uint8_t> zeros((size_t) (Z + 1) * fb, 0);
                if (R.push(flush ? (const void *) zeros.data() : (const void *) ((const uint8_t *) data + (size_t) T * fb), F, made.data()) != n_new) { ret = -1; bad = true; break; }
                R.ring_write(r_w, made.data(), n_new);
            }
            if (!flush) T += F;
            n_out += n_new; r_w += n_new; since += n_new;
        }
        if (bad) break;
        if (where == 1 && (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess)) break;
        if (!image()) break;
        ret = n_images;
    } while (false);
    if (d_in) (void) hipFree(d_in);
    if (d_zero) (void) hipFree(d_zero);
    if (d_img) (void) hipFree(d_img);
    if (d_taps) (void) hipFree(d_taps);
    return ret;
}

// The windows of n_sessions (<= 8) sessions in ONE launch of k_stream_window.  Every session reads its own device copy of `ring` (cap floats)
// that starts src_off[i] floats (0 .. 3) behind a 16-byte boundary, through pieces slot[i][4] / plen[i][4], and writes to a destination
// dst_off[i] floats (0 .. 3) behind a 16-byte boundary.  `out` receives, per session, `row` floats: [guard + dst_off][window][NaN to the end];
// everything but the window was NaN before the launch.  where = 0: wa_stream_ref's gather instead of the kernel, into the same layout.
// Returns 0, -1 refused arguments, -2 a HIP call failed, -3 the launcher refused.
ST_API int stest_window_run(int n_sessions, const float * ring, long long cap, const int * n_pieces, const int * slot, const int * plen, const int * src_off,
                            const int * dst_off, int where, float * out, long long row) {
    if (n_sessions <= 0 || n_sessions > WA_STREAM_SESSIONS || cap <= 0 || row % 4 != 0) return -1;
    const long long G = ST_GUARD, rs = (cap + 4 + 3) / 4 * 4;
    const float nan = std::nanf("");
    wa_stream_windows tab;
    memset(&tab, 0, sizeof(tab));
    for (int i = 0; i < n_sessions; ++i) {
        long long len = 0;
        if (n_pieces[i] <= 0 || n_pieces[i] > WA_STREAM_PIECES || src_off[i] < 0 || src_off[i] > 3 || dst_off[i] < 0 || dst_off[i] > 3) return -1;
        for (int q = 0; q < n_pieces[i]; ++q) {
            const long long s = slot[4 * i + q], l = plen[4 * i + q];
            if (s < 0 || l <= 0 || s + l > cap) return -1;             // the bounds the session checks before it launches
            len += l;
        }
        if (G + dst_off[i] + len + G > row) return -1;
        tab.w[i].len = (int32_t) len; tab.w[i].n_pieces = n_pieces[i];
        for (int q = 0; q < n_pieces[i]; ++q) { tab.w[i].slot[q] = slot[4 * i + q]; tab.w[i].plen[q] = plen[4 * i + q]; }
    }
    for (long long i = 0; i < n_sessions * row; ++i) out[i] = nan;
    if (where == 0) {
        wa_stream_ref R;
        R.ring.assign(ring, ring + cap);
        for (int i = 0; i < n_sessions; ++i) R.gather(n_pieces[i], slot + 4 * i, plen + 4 * i, out + (size_t) i * row + G + dst_off[i]);
        return 0;
    }
    float * d_rings = nullptr, * d_out = nullptr;
    int ret = -2;
    do {
        if (hipMalloc((void **) &d_rings, (size_t) n_sessions * rs * sizeof(float)) != hipSuccess ||
            hipMalloc((void **) &d_out, (size_t) n_sessions * row * sizeof(float)) != hipSuccess) break;
        if (hipMemcpy(d_out, out, (size_t) n_sessions * row * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) break;
        bool ok = true;
        for (int i = 0; i < n_sessions && ok; ++i) {
            float * r = d_rings + (size_t) i * rs + src_off[i];
            ok = hipMemcpy(r, ring, (size_t) cap * sizeof(float), hipMemcpyHostToDevice) == hipSuccess;
            tab.w[i].ring = r;
            tab.w[i].dst = d_out + (size_t) i * row + G + dst_off[i];
        }
        if (!ok) break;
        if (!wa_stream_window_launch(nullptr, tab, n_sessions)) { ret = -3; break; }
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) break;
        if (hipMemcpy(out, d_out, (size_t) n_sessions * row * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) break;
        ret = 0;
    } while (false);
    if (d_rings) (void) hipFree(d_rings);
    if (d_out) (void) hipFree(d_out);
    return ret;
}

// channels_kernels.hip - TEST INFRASTRUCTURE ONLY: C entry points around the launchers of wa_channels.hip (the two-channel kernels) and around
// the host functions of wa_channels.h they are held to, for tests/test_channels_kernels_gpu.py.  Linked against the product's own
// whisper-rust_amd/build/wa_channels_k.o (whisper-rust_amd/Makefile, target `channels_harness`), so the kernels under test are the ones
// libwhisper.so ships.  Launches go to the null stream.
#include "wa_channels.h"

#include <hip/hip_runtime.h>

#include <cstring>

#define CT_API extern "C" __attribute__((visibility("default")))

CT_API long long ctest_n_out(long long n_frames, int rate) { return wa_audio_n_out(n_frames, rate); }
CT_API long long ctest_stride(long long n_out) { return wa_ch_stride(n_out); }

// wa_ch_split_ref; `out` holds 2 * ctest_stride(n_out) floats, plane c at out + c * stride
CT_API long long ctest_split_ref(const void * data, long long n_frames, int rate, int format, float * out) {
    return wa_ch_split_ref(data, n_frames, rate, format, nullptr, out, wa_ch_stride(wa_audio_n_out(n_frames, rate)));
}

// The split kernels on a DEVICE copy of `data` that starts `offset` bytes behind a 256-byte boundary; `out` (host, 2 * stride floats) receives the
// two planes.  The device output buffer is filled with a mark first: `guard` floats in front of plane 0 and behind plane 1, and the floats
// between a plane's end and the stride, are checked to be untouched.  Returns the sample count per plane, or
// -1 refused arguments, -2 a HIP call failed, -3 the launcher did not take the shape, -4 a value outside the planes changed.
CT_API long long ctest_split_run(const void * data, long long n_frames, int rate, int format, int offset, float * out) {
    if (!wa_ch_args_ok(data, n_frames, rate, format) || offset < 0 || offset > 255) return -1;
    wa_audio_plan p;
    wa_audio_plan_make(rate, p);
    const long long n_out = wa_audio_n_out(n_frames, rate), stride = wa_ch_stride(n_out);
    const size_t bytes = (size_t) n_frames * (format == WA_AUDIO_I16 ? 4 : 8);
    const size_t guard = 64;
    uint8_t * d_in = nullptr;
    float * d_out = nullptr, * d_taps = nullptr;
    long long ret = -2;
    std::vector<float> taps, host((size_t) (2 * stride) + 2 * guard);
    const float mark = -12345.5f;
    for (auto & v : host) v = mark;
    do {
        if (hipMalloc((void **) &d_in, bytes + 512) != hipSuccess || hipMalloc((void **) &d_out, host.size() * sizeof(float)) != hipSuccess) break;
        if (bytes && hipMemcpy(d_in + offset, data, bytes, hipMemcpyHostToDevice) != hipSuccess) break;
        if (hipMemcpy(d_out, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) break;
        if (p.K) {
            wa_audio_taps(p, taps);
            if (hipMalloc((void **) &d_taps, taps.size() * sizeof(float)) != hipSuccess) break;
            if (hipMemcpy(d_taps, taps.data(), taps.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) break;
        }
        if (!wa_ch_split_launch(nullptr, d_in + offset, n_frames, format, p, d_taps, n_out, stride, d_out + guard)) { ret = -3; break; }
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) break;
        if (hipMemcpy(host.data(), d_out, host.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) break;
        ret = n_out;
        for (size_t i = 0; i < guard; ++i)
            if (host[i] != mark || host[guard + (size_t) (2 * stride) + i] != mark) ret = -4;
        for (int c = 0; c < 2; ++c)
            for (long long i = n_out; i < stride; ++i)
                if (host[guard + (size_t) (c * stride + i)] != mark) ret = -4;
        if (stride > 0) memcpy(out, host.data() + guard, (size_t) (2 * stride) * sizeof(float));
    } while (false);
    if (d_in) (void) hipFree(d_in);
    if (d_out) (void) hipFree(d_out);
    if (d_taps) (void) hipFree(d_taps);
    return ret;
}

// wa_ch_energy_ref over two planes of n samples `stride` apart: energy[2 i + c] of spans[2 i], spans[2 i + 1]
CT_API void ctest_energy_ref(const float * planes, long long n, long long stride, const long long * spans, int n_spans, double * energy) {
    for (int i = 0; i < n_spans; ++i)
        for (int c = 0; c < 2; ++c) energy[2 * i + c] = wa_ch_energy_ref(planes + c * stride, n, spans[2 * i], spans[2 * i + 1]);
}

// k_channel_energy on a device copy of the planes, ONE launch for all spans; 0, or -2 a HIP call failed, -3 the launcher refused
CT_API int ctest_energy_run(const float * planes, long long n, long long stride, const long long * spans, int n_spans, double * energy) {
    if (n < 0 || stride < n || n_spans < 0) return -1;
    if (n_spans == 0) return 0;
    float * d_planes = nullptr;
    long long * d_spans = nullptr;
    double * d_energy = nullptr;
    int ret = -2;
    const size_t pb = (size_t) (2 * stride) * sizeof(float), sb = (size_t) n_spans * 2 * sizeof(long long), eb = (size_t) n_spans * 2 * sizeof(double);
    do {
        if (hipMalloc((void **) &d_planes, pb + 256) != hipSuccess || hipMalloc((void **) &d_spans, sb) != hipSuccess ||
            hipMalloc((void **) &d_energy, eb) != hipSuccess) break;
        if (pb && hipMemcpy(d_planes, planes, pb, hipMemcpyHostToDevice) != hipSuccess) break;
        if (hipMemcpy(d_spans, spans, sb, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d_energy, 0xff, eb) != hipSuccess) break;
        if (!wa_ch_energy_launch(nullptr, d_planes, n, stride, d_spans, n_spans, d_energy)) { ret = -3; break; }
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) break;
        if (hipMemcpy(energy, d_energy, eb, hipMemcpyDeviceToHost) != hipSuccess) break;
        ret = 0;
    } while (false);
    if (d_planes) (void) hipFree(d_planes);
    if (d_spans) (void) hipFree(d_spans);
    if (d_energy) (void) hipFree(d_energy);
    return ret;
}

// audio_kernels.hip - TEST INFRASTRUCTURE ONLY: C entry points around the launcher of wa_audio.hip (the audio front end's kernels) and around
// the host functions of wa_audio.h they are held to, for tests/test_audio_kernels_gpu.py.  Linked against the product's own
// whisper-rust_amd/build/wa_audio_k.o (whisper-rust_amd/Makefile, target `audio_harness`), so the kernels under test are the ones
// libwhisper.so ships.  Launches go to the null stream.
#include "wa_audio.h"

#include <hip/hip_runtime.h>

#include <cstring>

#define AT_API extern "C" __attribute__((visibility("default")))

// wa_audio_ref; `out` holds atest_n_out(n_frames, rate) floats
AT_API long long atest_n_out(long long n_frames, int rate) { return wa_audio_n_out(n_frames, rate); }
AT_API long long atest_ref(const void * data, long long n_frames, int channels, int rate, int format, float * out) {
    return wa_audio_ref(data, n_frames, channels, rate, format, nullptr, out);
}

// The kernels on a DEVICE copy of `data` that starts `offset` bytes behind a 256-byte boundary; `out` (host) receives the samples, and
// `guard` floats on either side of the device output buffer are checked to be untouched.  Returns the sample count, or
// -1 refused arguments, -2 a HIP call failed, -3 the launcher did not take the shape, -4 a guard value changed.
AT_API long long atest_run(const void * data, long long n_frames, int channels, int rate, int format, int offset, float * out) {
    if (!wa_audio_args_ok(data, n_frames, channels, rate, format) || offset < 0 || offset > 255) return -1;
    wa_audio_plan p;
    wa_audio_plan_make(rate, p);
    const long long n_out = wa_audio_n_out(n_frames, rate);
    const size_t bytes = (size_t) n_frames * channels * (format == WA_AUDIO_I16 ? 2 : 4);
    const size_t guard = 64;
    uint8_t * d_in = nullptr;
    float * d_out = nullptr, * d_taps = nullptr;
    long long ret = -2;
    std::vector<float> taps, host((size_t) n_out + 2 * guard);
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
        if (!wa_audio_launch(nullptr, d_in + offset, n_frames, channels, format, p, d_taps, n_out, d_out + guard)) { ret = -3; break; }
        if (hipDeviceSynchronize() != hipSuccess || hipGetLastError() != hipSuccess) break;
        if (hipMemcpy(host.data(), d_out, host.size() * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) break;
        ret = n_out;
        for (size_t i = 0; i < guard; ++i)
            if (host[i] != mark || host[guard + (size_t) n_out + i] != mark) ret = -4;
        if (n_out > 0) memcpy(out, host.data() + guard, (size_t) n_out * sizeof(float));
    } while (false);
    if (d_in) (void) hipFree(d_in);
    if (d_out) (void) hipFree(d_out);
    if (d_taps) (void) hipFree(d_taps);
    return ret;
}

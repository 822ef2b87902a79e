// audio_math.cpp - TEST INFRASTRUCTURE ONLY: the audio front end's host code (whisper-rust_amd/csrc/wa_audio.h) behind a command file,
// for tests/test_audio_math.py.  g++ alone: no HIP, no device.  Built a second time with -fsanitize=address,undefined and run stand-alone.
//
// usage: audio_math COMMANDS      one command per line:
//   plan RATE                                      -> "plan ok L M K span" | "plan refused"
//   nout N_FRAMES RATE                             -> "nout N"
//   taps RATE OUT                                  -> "taps L M K", the table as raw F32 into OUT
//   ref RATE FORMAT CHANNELS N_FRAMES IN OUT VAR   -> "ref N", N raw F32 into OUT; IN holds the interleaved samples
//        VAR 0: wa_audio_ref itself.  1: the driver's own loop over the same taps (must equal 0 bit for bit).  Deliberately WRONG loops,
//        to show that the expected values tell them apart: 2 phase off by one, 3 taps reversed within a phase, 4 i0 rounded up (2 and 4
//        are the right loop where L == 1: one phase, t / L exact).
#include "wa_audio.h"

#include <cstdio>
#include <cstring>
#include <string>

static bool read_file(const char * path, std::vector<char> & buf) {
    FILE * f = fopen(path, "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize((size_t) n);
    const bool ok = n == 0 || fread(buf.data(), 1, (size_t) n, f) == (size_t) n;
    fclose(f);
    return ok;
}

static bool write_file(const char * path, const float * v, size_t n) {
    FILE * f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = n == 0 || fwrite(v, sizeof(float), n, f) == n;
    fclose(f);
    return ok;
}

static int64_t variant_loop(const void * data, int64_t n_frames, int channels, int rate, int format, int var, std::vector<float> & out) {
    wa_audio_plan p;
    if (!wa_audio_args_ok(data, n_frames, channels, rate, format) || !wa_audio_plan_make(rate, p) || !p.K) return -1;
    std::vector<float> taps;
    wa_audio_taps(p, taps);
    const int64_t n_out = wa_audio_n_out(n_frames, rate);
    out.assign((size_t) n_out, 0.0f);
    for (int64_t n = 0; n < n_out; ++n) {
        const int64_t t = n * p.M;
        int64_t ph = t % p.L, i0 = t / p.L;
        if (var == 2) ph = (ph + 1) % p.L;
        if (var == 4) i0 = (t + p.L - 1) / p.L;
        float acc = 0.0f;
        for (int k = 0; k < p.K; ++k) {
            const int64_t i = i0 - p.K / 2 + 1 + k;
            const float x = i >= 0 && i < n_frames ? wa_audio_frame(data, i, channels, format) : 0.0f;
            const float h = taps[(size_t) ph * p.K + (var == 3 ? p.K - 1 - k : k)];
            acc = std::fmaf(h, x, acc);
        }
        out[(size_t) n] = acc;
    }
    return n_out;
}

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: audio_math COMMANDS\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        char cmd[16] = "", in[1024] = "", outp[1024] = "";
        long long n_frames = 0;
        int rate = 0, format = 0, channels = 0, var = 0;
        if (sscanf(line, "%15s", cmd) != 1) continue;
        if (!strcmp(cmd, "plan") && sscanf(line, "%*s %d", &rate) == 1) {
            wa_audio_plan p;
            if (wa_audio_plan_make(rate, p)) printf("plan ok %d %d %d %d\n", p.L, p.M, p.K, wa_audio_span(p));
            else printf("plan refused\n");
        } else if (!strcmp(cmd, "nout") && sscanf(line, "%*s %lld %d", &n_frames, &rate) == 2) {
            printf("nout %lld\n", (long long) wa_audio_n_out(n_frames, rate));
        } else if (!strcmp(cmd, "taps") && sscanf(line, "%*s %d %1023s", &rate, outp) == 2) {
            wa_audio_plan p;
            if (!wa_audio_plan_make(rate, p)) { fprintf(stderr, "taps: rate %d refused\n", rate); return 1; }
            std::vector<float> taps;
            wa_audio_taps(p, taps);
            if (!write_file(outp, taps.data(), taps.size())) { fprintf(stderr, "cannot write %s\n", outp); return 1; }
            printf("taps %d %d %d\n", p.L, p.M, p.K);
        } else if (!strcmp(cmd, "ref") && sscanf(line, "%*s %d %d %d %lld %1023s %1023s %d", &rate, &format, &channels, &n_frames, in, outp, &var) == 7) {
            std::vector<char> buf;
            if (!read_file(in, buf)) { fprintf(stderr, "cannot read %s\n", in); return 1; }
            const size_t need = (size_t) (n_frames > 0 ? n_frames : 0) * (size_t) (channels > 0 ? channels : 0) * (format == WA_AUDIO_I16 ? 2 : 4);
            if (buf.size() < need) { fprintf(stderr, "%s is too short\n", in); return 1; }
            const void * data = n_frames > 0 ? (const void *) buf.data() : nullptr;
            std::vector<float> out;
            int64_t n;
            if (var == 0) {
                const int64_t n_out = wa_audio_n_out(n_frames, rate);
                out.assign((size_t) (n_out > 0 ? n_out : 0), 0.0f);
                n = wa_audio_ref(data, n_frames, channels, rate, format, nullptr, out.data());
            } else {
                n = variant_loop(data, n_frames, channels, rate, format, var, out);
            }
            if (n >= 0 && !write_file(outp, out.data(), (size_t) n)) { fprintf(stderr, "cannot write %s\n", outp); return 1; }
            printf("ref %lld\n", (long long) n);
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 1;
        }
    }
    fclose(f);
    return 0;
}

// audio_formats_math.cpp - TEST INFRASTRUCTURE ONLY: the host code of the audio front end's sample formats and of the WAV header parser
// (whisper-rust_amd/csrc/wa_audio.h, wa_channels.h, wa_stream.h, wa_wav.h) behind a command file, for tests/test_audio_formats_math.py.
// g++ alone: no HIP, no device.  Built a second time with -fsanitize=address,undefined and run stand-alone.
//
// usage: audio_formats_math COMMANDS      one command per line:
//   g711                                                  -> "ulaw e0 .. e255" and "alaw e0 .. e255": both expansions, every code
//   ref RATE FORMAT CHANNELS N_FRAMES OFFSET IN OUT       -> "ref N", wa_audio_ref's N raw F32 into OUT.  The samples of IN are copied OFFSET
//                                                            bytes into a heap block that ends with them: the pointer is misaligned and a read
//                                                            past the last sample is the sanitiser's to see.
//   split RATE FORMAT N_FRAMES OFFSET IN OUT              -> "split N", wa_ch_split_ref's plane 0 then plane 1 (N each) into OUT
//   stream RATE FORMAT CHANNELS N_FRAMES IN OUT P1,P2,..  -> "stream N", wa_stream_ref fed packets of P1, P2, ... frames in turn (round and round) until
//                                                            N_FRAMES are in, then flushed: every output in order into OUT
//   wav IN                                                -> "wav RC data_offset n_frames channels rate format bits" of wa_wav_parse on the image IN;
//                                                            the record starts as -7 in every field: a refusal must leave it so
//   wavargs IN                                            -> "wavargs RC RC RC RC": null image, null out, size 11, size -1
#include "wa_channels.h"
#include "wa_stream.h"
#include "wa_wav.h"

#include <cstdio>
#include <cstdlib>
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

// the first `need` bytes of IN, `offset` bytes into a heap block of exactly offset + need bytes
struct shifted {
    char * block = nullptr;
    const void * data = nullptr;
    bool load(const char * path, size_t need, int offset) {
        std::vector<char> buf;
        if (!read_file(path, buf) || buf.size() < need) { fprintf(stderr, "cannot read %zu bytes of %s\n", need, path); return false; }
        block = (char *) malloc(need + (size_t) offset + 1);       // + 1: malloc(0) may give null
        if (!block) return false;
        if (need) memcpy(block + offset, buf.data(), need);
        data = need ? block + offset : nullptr;
        return true;
    }
    ~shifted() { free(block); }
};

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: audio_formats_math COMMANDS\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        char cmd[16] = "", in[1024] = "", outp[1024] = "", packets[1024] = "";
        long long n_frames = 0;
        int rate = 0, format = 0, channels = 0, offset = 0;
        if (sscanf(line, "%15s", cmd) != 1) continue;
        if (!strcmp(cmd, "g711")) {
            printf("ulaw");
            for (unsigned b = 0; b < 256; ++b) printf(" %d", wa_audio_ulaw(b));
            printf("\nalaw");
            for (unsigned b = 0; b < 256; ++b) printf(" %d", wa_audio_alaw(b));
            printf("\n");
        } else if (!strcmp(cmd, "ref") && sscanf(line, "%*s %d %d %d %lld %d %1023s %1023s", &rate, &format, &channels, &n_frames, &offset, in, outp) == 7) {
            shifted s;
            if (n_frames < 0 || !s.load(in, (size_t) n_frames * wa_audio_frame_bytes(format, channels), offset)) return 1;
            const int64_t n_out = wa_audio_n_out(n_frames, rate);
            std::vector<float> out((size_t) (n_out > 0 ? n_out : 0), 0.0f);
            const int64_t n = wa_audio_ref(s.data, n_frames, channels, rate, format, nullptr, out.data());
            if (n >= 0 && !write_file(outp, out.data(), (size_t) n)) { fprintf(stderr, "cannot write %s\n", outp); return 1; }
            printf("ref %lld\n", (long long) n);
        } else if (!strcmp(cmd, "split") && sscanf(line, "%*s %d %d %lld %d %1023s %1023s", &rate, &format, &n_frames, &offset, in, outp) == 6) {
            shifted s;
            if (n_frames < 0 || !s.load(in, (size_t) n_frames * wa_audio_frame_bytes(format, 2), offset)) return 1;
            const int64_t n_out = wa_audio_n_out(n_frames, rate);
            std::vector<float> out((size_t) (n_out > 0 ? 2 * n_out : 0), 0.0f);
            const int64_t n = wa_ch_split_ref(s.data, n_frames, rate, format, nullptr, out.data(), n_out);
            if (n >= 0 && !write_file(outp, out.data(), (size_t) (2 * n))) { fprintf(stderr, "cannot write %s\n", outp); return 1; }
            printf("split %lld\n", (long long) n);
        } else if (!strcmp(cmd, "stream") && sscanf(line, "%*s %d %d %d %lld %1023s %1023s %1023s", &rate, &format, &channels, &n_frames, in, outp, packets) == 7) {
            shifted s;
            const size_t fb = wa_audio_frame_bytes(format, channels);
            if (n_frames < 0 || !s.load(in, (size_t) n_frames * fb, 1)) return 1;
            std::vector<long long> sizes;
            for (char * tok = strtok(packets, ","); tok; tok = strtok(nullptr, ",")) sizes.push_back(atoll(tok));
            wa_stream_ref R;
            if (sizes.empty() || !R.init(rate, channels, format, 0)) { printf("stream -1\n"); continue; }
            std::vector<float> all, out;
            long long fed = 0;
            for (size_t k = 0; fed < n_frames; ++k) {
                const long long n = std::min(std::max(sizes[k % sizes.size()], 1LL), n_frames - fed);
                out.assign((size_t) std::max<int64_t>(R.n_new(n), 1), 0.0f);
                const int64_t made = R.push((const char *) s.data + (size_t) fed * fb, n, out.data());
                all.insert(all.end(), out.begin(), out.begin() + made);
                fed += n;
            }
            out.assign((size_t) wa_stream_flush_frames(R.ap) * WA_AUDIO_MAX_L + 16, 0.0f);
            const int64_t made = R.flush(out.data());
            all.insert(all.end(), out.begin(), out.begin() + made);
            if (!write_file(outp, all.data(), all.size())) { fprintf(stderr, "cannot write %s\n", outp); return 1; }
            printf("stream %zu\n", all.size());
        } else if (!strcmp(cmd, "wav") && sscanf(line, "%*s %1023s", in) == 1) {
            shifted s;
            std::vector<char> buf;
            if (!read_file(in, buf) || !s.load(in, buf.size(), 1)) return 1;
            wa_wav_info w = { -7, -7, -7, -7, -7, -7 };
            const int rc = wa_wav_parse(s.data ? s.data : s.block, (int64_t) buf.size(), &w);
            printf("wav %d %lld %lld %d %d %d %d\n", rc, (long long) w.data_offset, (long long) w.n_frames, w.channels, w.sample_rate, w.format, w.bits);
        } else if (!strcmp(cmd, "wavargs") && sscanf(line, "%*s %1023s", in) == 1) {
            std::vector<char> buf;
            if (!read_file(in, buf)) return 1;
            wa_wav_info w = { -7, -7, -7, -7, -7, -7 };
            const int a = wa_wav_parse(nullptr, (int64_t) buf.size(), &w), b = wa_wav_parse(buf.data(), (int64_t) buf.size(), nullptr);
            const int c = wa_wav_parse(buf.data(), 11, &w), d = wa_wav_parse(buf.data(), -1, &w);
            printf("wavargs %d %d %d %d%s\n", a, b, c, d, w.format == -7 && w.data_offset == -7 ? "" : " (record touched)");
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 1;
        }
    }
    fclose(f);
    return 0;
}

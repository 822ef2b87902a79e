// channels_math.cpp - TEST INFRASTRUCTURE ONLY: the host code of the two-channel calls (whisper-rust_amd/csrc/wa_channels.h, wa_audio.h) behind a
// command file, for tests/test_channels_math.py.  g++ alone: no HIP, no device.
//
// usage: channels_math COMMANDS      one command per line:
//   split RATE FORMAT N_FRAMES IN OUT0 OUT1      -> "split N STRIDE", the two planes of wa_ch_split_ref as raw F32 (N each); IN: interleaved stereo
//   mono RATE FORMAT N_FRAMES IN C OUT           -> "mono N", wa_audio_ref on channel C of IN extracted here and presented as a mono recording
//   energy IN OUT A B [A B ...]                  -> "energy K", wa_ch_energy_ref of the plane IN (raw F32) over every [A, B) as raw F64 into OUT
//   label E0 E1 RATIO                            -> "label 0|1|-1"      (numbers in any strtod form, hex floats included)
//   cs T N_SAMPLES                               -> "cs S"              wa_ch_cs_to_sample
//   gate E_OWN E_OTHER G                         -> "gate 0|1"          1: dropped
//   merge N0 (T0 T1)*N0 N1 (T0 T1)*N1            -> "merge" then "C INDEX T0 T1" per segment in merged order, all on one line
//   const                                        -> "const TILE LDS LANES ALIGN"
//   span RATE                                    -> "span S L K"        wa_ch_span and the plan
#include "wa_channels.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

static bool read_file(const std::string & path, std::vector<char> & buf) {
    FILE * f = fopen(path.c_str(), "rb");
    if (!f) return false;
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize((size_t) n);
    const bool ok = n == 0 || fread(buf.data(), 1, (size_t) n, f) == (size_t) n;
    fclose(f);
    return ok;
}

static bool write_file(const std::string & path, const void * v, size_t bytes) {
    FILE * f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || fwrite(v, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

static double num(const std::string & s) { return strtod(s.c_str(), nullptr); }

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: channels_math COMMANDS\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[1 << 16];
    while (fgets(line, sizeof line, f)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "split") {
            int rate, fmt; long long n; std::string ip, o0, o1;
            in >> rate >> fmt >> n >> ip >> o0 >> o1;
            std::vector<char> buf;
            if (!read_file(ip, buf) || buf.size() != (size_t) n * (fmt == WA_AUDIO_I16 ? 4 : 8)) { fprintf(stderr, "bad input %s\n", ip.c_str()); return 1; }
            const int64_t n_out = wa_audio_n_out(n, rate), stride = wa_ch_stride(n_out < 0 ? 0 : n_out);
            std::vector<float> out((size_t) (2 * stride) + 1, 0.0f);
            const int64_t got = wa_ch_split_ref(buf.data(), n, rate, fmt, nullptr, out.data(), stride);
            if (got >= 0 && (!write_file(o0, out.data(), (size_t) got * 4) || !write_file(o1, out.data() + stride, (size_t) got * 4))) return 1;
            printf("split %lld %lld\n", (long long) got, (long long) stride);
        } else if (cmd == "mono") {
            int rate, fmt, c; long long n; std::string ip, op;
            in >> rate >> fmt >> n >> ip >> c >> op;
            std::vector<char> buf;
            if (!read_file(ip, buf) || buf.size() != (size_t) n * (fmt == WA_AUDIO_I16 ? 4 : 8)) { fprintf(stderr, "bad input %s\n", ip.c_str()); return 1; }
            const size_t w = fmt == WA_AUDIO_I16 ? 2 : 4;
            std::vector<char> mono((size_t) n * w + 1);
            for (long long i = 0; i < n; ++i) memcpy(mono.data() + (size_t) i * w, buf.data() + ((size_t) (2 * i + c)) * w, w);
            const int64_t n_out = wa_audio_n_out(n, rate);
            std::vector<float> out((size_t) (n_out < 0 ? 0 : n_out) + 1, 0.0f);
            const int64_t got = wa_audio_ref(mono.data(), n, 1, rate, fmt, nullptr, out.data());
            if (got >= 0 && !write_file(op, out.data(), (size_t) got * 4)) return 1;
            printf("mono %lld\n", (long long) got);
        } else if (cmd == "energy") {
            std::string ip, op;
            in >> ip >> op;
            std::vector<char> buf;
            if (!read_file(ip, buf) || buf.size() % 4 != 0) { fprintf(stderr, "bad input %s\n", ip.c_str()); return 1; }
            std::vector<float> x(buf.size() / 4 + 1);
            memcpy(x.data(), buf.data(), buf.size());
            std::vector<double> e;
            long long a, b;
            while (in >> a >> b) e.push_back(wa_ch_energy_ref(x.data(), (int64_t) (buf.size() / 4), a, b));
            if (!write_file(op, e.data(), e.size() * 8)) return 1;
            printf("energy %zu\n", e.size());
        } else if (cmd == "label") {
            std::string a, b, r;
            in >> a >> b >> r;
            printf("label %d\n", wa_ch_label(num(a), num(b), num(r)));
        } else if (cmd == "cs") {
            long long t, n;
            in >> t >> n;
            printf("cs %lld\n", (long long) wa_ch_cs_to_sample(t, n));
        } else if (cmd == "gate") {
            std::string a, b, g;
            in >> a >> b >> g;
            printf("gate %d\n", wa_ch_gate_drops(num(a), num(b), num(g)) ? 1 : 0);
        } else if (cmd == "merge") {
            std::vector<wa_ch_item> items[2];
            for (int c = 0; c < 2; ++c) {
                int n = 0;
                in >> n;
                for (int i = 0; i < n; ++i) { long long t0, t1; in >> t0 >> t1; items[c].push_back({ t0, t1, -1, -1 }); }
            }
            printf("merge");
            for (const wa_ch_item & it : wa_ch_merge(items)) printf(" %d %d %lld %lld", it.channel, it.index, (long long) it.t0, (long long) it.t1);
            printf("\n");
        } else if (cmd == "const") {
            printf("const %d %d %d %d\n", WA_CH_TILE, WA_CH_LDS, WA_CH_LANES, WA_CH_ALIGN);
        } else if (cmd == "span") {
            int rate;
            in >> rate;
            wa_audio_plan p;
            if (!wa_audio_plan_make(rate, p)) printf("span refused\n");
            else printf("span %d %d %d\n", wa_ch_span(p), p.L, p.K);
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    fclose(f);
    return 0;
}

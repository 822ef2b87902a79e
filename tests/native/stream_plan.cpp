// stream_plan.cpp - TEST INFRASTRUCTURE ONLY: the streaming sessions' host code (whisper-rust_amd/csrc/wa_stream.h) behind a command file,
// for tests/test_stream_plan_math.py.  g++ alone: no HIP, no device.  Built a second time with -fsanitize=address,undefined and run stand-alone.
//
// usage: stream_plan COMMANDS      one command per line:
//   sizes STEP LEN KEEP                            -> "sizes ok n_step n_len n_keep n_new_line" | "sizes refused"
//   plan STEP LEN KEEP N_WINDOWS VAR               -> N_WINDOWS lines "win take len commit n_ranges start": n_step samples arrive before each window
//   drop STEP LEN KEEP PENDING                     -> two windows as above, then PENDING samples arrive and a step is asked for:
//                                                     "drop dropped ran", then n_step more arrive (only after a drop) and a step is asked for:
//                                                     "win take len commit n_ranges start0 len0 start1 len1"
//   ring R0 LEN CAP                                -> "ring n slot0 len0 slot1 len1"
//   final RATE T VAR                               -> "final N"
//   whole RATE FORMAT CHANNELS N_FRAMES IN OUT     -> "whole N": wa_audio_ref on the whole recording, N raw F32 into OUT
//   push RATE FORMAT CHANNELS N_FRAMES IN SPLIT OUT COUNTS VAR
//        -> "push N": the recording fed through wa_stream_ref in the packets SPLIT lists (raw int64 frame counts), then flushed; every push
//           writes what it made final into a ring of 4096 samples at the write head, and the same range is gathered back through
//           wa_stream_ring_pieces: the concatenation of the gathers goes to OUT (N raw F32), the output count after every push and after the
//           flush to COUNTS (raw int64).
//   VAR 0: the header's rule.  Deliberately WRONG, to show that the expected values tell them apart: 1 an output released one frame early,
//   2 a carry one frame short (push), 3 the commit taken on iter % n_new_line == 1, 4 take computed from n_len alone (plan).
#include "wa_stream.h"

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

static bool write_file(const char * path, const void * v, size_t bytes) {
    FILE * f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = bytes == 0 || fwrite(v, 1, bytes, f) == bytes;
    fclose(f);
    return ok;
}

static void print_win(const wa_stream_step & s, bool both) {
    printf("win %d %d %d %d %lld", s.take, s.len, s.commit ? 1 : 0, (int) s.ranges.size(), (long long) s.ranges[0].start);
    if (both) printf(" %lld %lld %lld", (long long) s.ranges[0].len, (long long) (s.ranges.size() > 1 ? s.ranges[1].start : -1),
                     (long long) (s.ranges.size() > 1 ? s.ranges[1].len : -1));
    printf("\n");
}

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: stream_plan COMMANDS\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[8192];
    while (fgets(line, sizeof line, f)) {
        char cmd[16] = "", in[1024] = "", split[1024] = "", outp[1024] = "", counts[1024] = "";
        long long a = 0, b = 0, c = 0;
        int step = 0, len = 0, keep = 0, n = 0, var = 0, rate = 0, format = 0, channels = 0;
        if (sscanf(line, "%15s", cmd) != 1) continue;
        if (!strcmp(cmd, "sizes") && sscanf(line, "%*s %d %d %d", &step, &len, &keep) == 3) {
            wa_stream_sizes z;
            if (wa_stream_sizes_make(step, len, keep, z)) printf("sizes ok %d %d %d %d\n", z.n_step, z.n_len, z.n_keep, z.n_new_line);
            else printf("sizes refused\n");
        } else if (!strcmp(cmd, "plan") && sscanf(line, "%*s %d %d %d %d %d", &step, &len, &keep, &n, &var) == 5) {
            wa_stream_plan P;
            if (!wa_stream_sizes_make(step, len, keep, P.z)) { fprintf(stderr, "plan: sizes refused\n"); return 1; }
            for (int k = 0; k < n; ++k) {
                wa_stream_step s;
                P.r_w += P.z.n_step;
                if (!wa_stream_next(P, false, s, var)) { fprintf(stderr, "plan: no window due\n"); return 1; }
                print_win(s, false);
            }
        } else if (!strcmp(cmd, "drop") && sscanf(line, "%*s %d %d %d %lld", &step, &len, &keep, &a) == 4) {
            wa_stream_plan P;
            P.drop_late = true;
            if (!wa_stream_sizes_make(step, len, keep, P.z)) { fprintf(stderr, "drop: sizes refused\n"); return 1; }
            wa_stream_step s;
            for (int k = 0; k < 2; ++k) { P.r_w += P.z.n_step; if (!wa_stream_next(P, false, s)) { fprintf(stderr, "drop: no window due\n"); return 1; } }
            P.r_w += a;
            const bool ran = wa_stream_next(P, false, s);
            printf("drop %lld %d\n", (long long) s.dropped, ran ? 1 : 0);
            if (!ran) { P.r_w += P.z.n_step; if (!wa_stream_next(P, false, s)) { fprintf(stderr, "drop: no window after the drop\n"); return 1; } }
            print_win(s, true);
        } else if (!strcmp(cmd, "ring") && sscanf(line, "%*s %lld %lld %lld", &a, &b, &c) == 3) {
            int32_t slot[2] = { -1, -1 }, plen[2] = { -1, -1 };
            const int np = wa_stream_ring_pieces(a, b, c, slot, plen);
            printf("ring %d %d %d %d %d\n", np, slot[0], plen[0], slot[1], plen[1]);
        } else if (!strcmp(cmd, "final") && sscanf(line, "%*s %d %lld %d", &rate, &a, &var) == 3) {
            wa_audio_plan p;
            if (!wa_audio_plan_make(rate, p)) { fprintf(stderr, "final: rate refused\n"); return 1; }
            printf("final %lld\n", (long long) wa_stream_final(p, a, var));
        } else if (!strcmp(cmd, "whole") && sscanf(line, "%*s %d %d %d %lld %1023s %1023s", &rate, &format, &channels, &a, in, outp) == 6) {
            std::vector<char> x;
            if (!read_file(in, x)) { fprintf(stderr, "whole: cannot read %s\n", in); return 1; }
            std::vector<float> out((size_t) std::max<int64_t>(wa_audio_n_out(a, rate), 1));
            const int64_t got = wa_audio_ref(x.data(), a, channels, rate, format, nullptr, out.data());
            if (got < 0 || !write_file(outp, out.data(), (size_t) got * sizeof(float))) { fprintf(stderr, "whole: failed\n"); return 1; }
            printf("whole %lld\n", (long long) got);
        } else if (!strcmp(cmd, "push") && sscanf(line, "%*s %d %d %d %lld %1023s %1023s %1023s %1023s %d", &rate, &format, &channels, &a, in, split, outp,
                                                  counts, &var) == 9) {
            std::vector<char> x, sp;
            if (!read_file(in, x) || !read_file(split, sp)) { fprintf(stderr, "push: cannot read the inputs\n"); return 1; }
            const int64_t * packets = (const int64_t *) sp.data();
            const size_t n_packets = sp.size() / sizeof(int64_t);
            const int64_t cap = 4096;
            const size_t fb = (size_t) channels * (format == WA_AUDIO_I16 ? 2 : 4);
            wa_stream_ref R;
            if (!R.init(rate, channels, format, cap)) { fprintf(stderr, "push: refused\n"); return 1; }
            std::vector<float> all, made, back;
            std::vector<int64_t> cnt;
            int64_t fed = 0, r_w = 0;
            for (size_t k = 0; k <= n_packets; ++k) {           // the last round is the flush
                int64_t got;
                if (k < n_packets) {
                    const int64_t F = packets[k];
                    if (F < 0 || fed + F > a) { fprintf(stderr, "push: the split does not fit the recording\n"); return 1; }
                    made.assign((size_t) std::max<int64_t>(R.n_new(F, var), 1), 0.0f);
                    got = R.push(x.data() + (size_t) fed * fb, F, made.data(), var);
                    fed += F;
                } else {
                    if (fed != a) { fprintf(stderr, "push: the split covers %lld of %lld frames\n", (long long) fed, a); return 1; }
                    made.assign((size_t) std::max<int64_t>(R.n_new(wa_stream_flush_frames(R.ap)), 1), 0.0f);
                    got = R.flush(made.data());
                }
                if (got > cap) { fprintf(stderr, "push: a packet larger than the ring\n"); return 1; }
                R.ring_write(r_w, made.data(), got);
                int32_t slot[2], plen[2];
                const int np = wa_stream_ring_pieces(r_w, got, cap, slot, plen);
                back.assign((size_t) std::max<int64_t>(got, 1), 0.0f);
                R.gather(np, slot, plen, back.data());
                all.insert(all.end(), back.begin(), back.begin() + got);
                r_w += got;
                cnt.push_back(R.n_out);
            }
            if (!write_file(outp, all.data(), all.size() * sizeof(float)) || !write_file(counts, cnt.data(), cnt.size() * sizeof(int64_t))) {
                fprintf(stderr, "push: cannot write the outputs\n");
                return 1;
            }
            printf("push %zu\n", all.size());
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 1;
        }
    }
    fclose(f);
    return 0;
}

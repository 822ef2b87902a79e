// stream_vad_plan.cpp - TEST INFRASTRUCTURE ONLY: the incremental speech segmenter of live VAD sessions (whisper-rust_amd/csrc/wa_stream_vad.h)
// beside the offline rules it restates (wa_vad_segments_from_probs of wa_vad_host.cpp), behind a command file, for
// tests/test_stream_vad_math.py.  g++ alone: no HIP, no device.  Built a second time with -fsanitize=address,undefined and run stand-alone.
//
// usage: stream_vad_plan COMMANDS      one command per line:
//   run THRESHOLD MIN_SPEECH_MS MIN_SILENCE_MS MAX_SPEECH_S PAD_MS CAP_MS VAR PROBS
//        PROBS: raw F32, one probability per 512-sample window.  Prints
//          "params ok" | "params refused"                     wa_svad_params_ok (a refused set is still run: the variants need none)
//          "inc K SPLITS"                                     the segmenter fed window by window, then flushed
//          K x "START_CS END_CS SPLIT RAW_END WINDOW LEN"     WINDOW: the push that handed the segment out, -1 the flush; LEN: its utterance
//          "off M" and M x "START_CS END_CS"                  wa_vad_segments_from_probs on the whole sequence
//          "bound B"                                          wa_svad_delay_bound
//   raws (the same settings) RAWS
//        RAWS: raw int32: N_WINDOWS, then (start, end) pairs in samples - speeches as the first pass would push them, handed to the merge stage
//        directly (the first pass only makes multiples of 512: this is how a gap of exactly 3199 or 3200 samples is reached), then the flush.
//        Prints "inc K SPLITS" and the K lines as above.
//   VAR 0: the header's rule.  Deliberately WRONG, to show that the expected lists tell them apart: 1 the merge look-ahead one window short,
//   2 padding decided before the merge, 3 <= for < at 3200.
#include "wa_stream_vad.h"

#include <cstdio>
#include <cstring>

int main(int argc, char ** argv) {
    if (argc != 2) { fprintf(stderr, "usage: stream_vad_plan COMMANDS\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char line[4096];
    while (fgets(line, sizeof line, f)) {
        char cmd[16] = "", path[2048] = "";
        float thr = 0, max_s = 0;
        int min_speech = 0, min_silence = 0, pad = 0, cap_ms = 0, var = 0;
        if (sscanf(line, "%15s %f %d %d %f %d %d %d %2047s", cmd, &thr, &min_speech, &min_silence, &max_s, &pad, &cap_ms, &var, path) != 9 ||
            (strcmp(cmd, "run") != 0 && strcmp(cmd, "raws") != 0)) {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
        if (strcmp(cmd, "raws") == 0) {
            FILE * rf = fopen(path, "rb");
            if (!rf) { fprintf(stderr, "cannot open %s\n", path); return 2; }
            std::vector<int32_t> v;
            int32_t b[256];
            size_t n;
            while ((n = fread(b, sizeof(int32_t), 256, rf)) > 0) v.insert(v.end(), b, b + n);
            fclose(rf);
            if (v.empty() || v.size() % 2 != 1) { fprintf(stderr, "raws: N_WINDOWS and pairs expected\n"); return 2; }
            whisper_vad_params p;
            p.threshold = thr; p.min_speech_duration_ms = min_speech; p.min_silence_duration_ms = min_silence; p.max_speech_duration_s = max_s;
            p.speech_pad_ms = pad; p.samples_overlap = 0.1f;
            wa_svad_segmenter seg;
            seg.init(p, cap_ms, var);
            std::vector<wa_svad_out> out;
            for (size_t k = 1; k + 1 < v.size(); k += 2) seg.raw(v[k], v[k + 1], out);
            seg.n_probs = v[0];
            seg.flush((int64_t) v[0] * WA_VAD_WINDOW, out);
            printf("inc %d %lld\n", (int) out.size(), (long long) seg.splits);
            for (const wa_svad_out & o : out) printf("%lld %lld %d %d -1 %lld\n", (long long) o.seg.start, (long long) o.seg.end, o.split ? 1 : 0, o.raw_end,
                                                    (long long) wa_svad_range_of(o.seg, seg.T_end).len);
            continue;
        }
        FILE * pf = fopen(path, "rb");
        if (!pf) { fprintf(stderr, "cannot open %s\n", path); return 2; }
        std::vector<float> probs;
        float buf[1024];
        size_t got;
        while ((got = fread(buf, sizeof(float), 1024, pf)) > 0) probs.insert(probs.end(), buf, buf + got);
        fclose(pf);

        whisper_vad_params p;
        p.threshold = thr; p.min_speech_duration_ms = min_speech; p.min_silence_duration_ms = min_silence; p.max_speech_duration_s = max_s;
        p.speech_pad_ms = pad; p.samples_overlap = 0.1f;
        const char * why = nullptr;
        printf("params %s\n", wa_svad_params_ok(p, cap_ms, &why) ? "ok" : "refused");

        wa_svad_segmenter seg;
        seg.init(p, cap_ms, var);
        std::vector<wa_svad_out> out;
        std::vector<int> at;
        for (size_t i = 0; i < probs.size(); ++i) {
            seg.push(probs[i], out);
            while (at.size() < out.size()) at.push_back((int) i);
        }
        const int64_t T = (int64_t) probs.size() * WA_VAD_WINDOW;
        seg.flush(T, out);
        while (at.size() < out.size()) at.push_back(-1);
        printf("inc %d %lld\n", (int) out.size(), (long long) seg.splits);
        for (size_t k = 0; k < out.size(); ++k)
            printf("%lld %lld %d %d %d %lld\n", (long long) out[k].seg.start, (long long) out[k].seg.end, out[k].split ? 1 : 0, out[k].raw_end, at[k],
                   (long long) wa_svad_range_of(out[k].seg, seg.T_end).len);

        const std::vector<wa_vad_seg> off = wa_vad_segments_from_probs(probs.data(), (int) probs.size(), WA_VAD_WINDOW, p);
        printf("off %d\n", (int) off.size());
        for (const wa_vad_seg & g : off) printf("%lld %lld\n", (long long) g.start, (long long) g.end);
        printf("bound %d\n", wa_svad_delay_bound(p));
    }
    fclose(f);
    return 0;
}

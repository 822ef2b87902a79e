// long_plan.cpp - CPU driver of tests/test_long_plan_math.py: the chunk planner of whisper_amd_full_long (whisper-rust_amd/csrc/wa_long_plan.h)
// beside the function it must agree with, wa_vad_filter_audio (wa_vad_host.cpp).  No HIP, no device.
//   g++ -O2 -std=c++17 -mavx2 -mf16c -ffp-contract=off long_plan.cpp ../../whisper-rust_amd/csrc/wa_vad_host.cpp
//
// usage: long_plan <script>; one case per line:
//   <n_samples> <samples_overlap> <max_chunk_samples> <n_segs> <start cs> <end cs> ...
// answer: "plan <k>", then per chunk one line
//   "chunk <first> <count> <packed> L <length> <n> <p> <o> ... F <length> <n> <p> <o> ..."
// L: wa_vad_layout_make on the chunk's sub-list (length, table); F: wa_vad_filter_audio on the same sub-list over a ramp signal (length of the
// audio it returns, its table); then "whole L ... F ..." for the whole list, and "pieces <ok>": 1 when the sub-lists' pieces rebuild F's audio.
#include "../../whisper-rust_amd/csrc/wa_long_plan.h"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

static void print_table(const char * tag, size_t length, const std::vector<wa_vad_map_point> & t) {
    printf(" %s %zu %zu", tag, length, t.size());
    for (const auto & p : t) printf(" %lld %lld", (long long) p.processed_time, (long long) p.original_time);
}

// both statements for one list; returns whether the pieces rebuild the audio wa_vad_filter_audio returned
static bool both(const std::vector<wa_vad_seg> & segs, float overlap, const std::vector<float> & ramp, int n_samples) {
    std::vector<wa_long_piece> pieces;
    std::vector<wa_vad_map_point> lt, ft;
    std::vector<float> filtered;
    const int total = wa_vad_layout_make(segs.data(), (int) segs.size(), overlap, n_samples, &pieces, &lt);
    wa_vad_filter_audio(segs, overlap, ramp.data(), n_samples, filtered, ft);
    print_table("L", (size_t) total, lt);
    print_table("F", filtered.size(), ft);
    std::vector<float> rebuilt((size_t) total, 0.0f);
    long long at = 0;
    for (const auto & p : pieces) {
        if (p.dst < at || p.len <= 0 || p.dst + p.len > total || (p.src >= 0 && p.src + p.len > n_samples)) return false;
        if (p.src >= 0) memcpy(rebuilt.data() + p.dst, ramp.data() + p.src, (size_t) p.len * sizeof(float));
        at = p.dst + p.len;
    }
    return rebuilt.size() == filtered.size() && (rebuilt.empty() || memcmp(rebuilt.data(), filtered.data(), rebuilt.size() * sizeof(float)) == 0);
}

int main(int argc, char ** argv) {
    if (argc < 2) { fprintf(stderr, "usage: long_plan <script>\n"); return 2; }
    std::ifstream script(argv[1]);
    if (!script) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<float> ramp;
    std::string line;
    while (std::getline(script, line)) {
        std::istringstream ss(line);
        int n_samples = 0, cap = 0, n_segs = 0;
        float overlap = 0.0f;
        if (!(ss >> n_samples >> overlap >> cap >> n_segs)) continue;
        std::vector<wa_vad_seg> segs((size_t) n_segs);
        for (auto & s : segs) { long long a = 0, b = 0; ss >> a >> b; s.start = a; s.end = b; }
        if (!ss || n_samples <= 0) { printf("bad case\n"); return 1; }
        for (size_t i = ramp.size(); i < (size_t) n_samples; ++i) ramp.push_back((float) (i % 16777213u + 1));    // non-zero, exact in F32
        const std::vector<wa_long_chunk> plan = wa_long_plan(segs.data(), n_segs, n_samples, overlap, cap);
        printf("plan %zu\n", plan.size());
        bool ok = true;
        for (const auto & c : plan) {
            printf("chunk %d %d %d", c.first, c.count, c.packed);
            ok = both(std::vector<wa_vad_seg>(segs.begin() + c.first, segs.begin() + c.first + c.count), overlap, ramp, n_samples) && ok;
            printf("\n");
        }
        printf("whole");
        ok = both(segs, overlap, ramp, n_samples) && ok;
        printf("\npieces %d\n", ok ? 1 : 0);
    }
    return 0;
}

// tts_math.cpp - the snap pass of the heuristic token timestamps as it is now (a record per token from wa_tts_record_host, then wa_tts_finalise:
// whisper-rust_amd/csrc/wa_tts.h) against a literal copy of the pass it replaced, which walked the energy array itself.  g++ alone, no device.
// Usage: tts_math <cases>; seeded random time lines over random burst energies; exit 0 when every case agrees AND every branch was taken.
#include "wa_tts.h"

#include <cstdio>
#include <cstdlib>
#include <random>

struct old_timeline {       // wa_full.cpp's token_timeline before the records: snap(j) as it stood
    int n; int64_t seg_lo; std::vector<int64_t> lo, hi; const std::vector<float> & energy;
    float energy_at(int k) const { return energy[(size_t) std::min(std::max(k, 0), (int) energy.size() - 1)]; }
    int to_sample(int64_t t) const {
        const int smp = (int) (((t - seg_lo) * WA_TTS_RATE) / 100);
        return std::min(std::max(smp, 0), (int) energy.size() - 1);
    }
    int64_t to_time(int smp) const { return (100ll * smp) / WA_TTS_RATE + seg_lo; }
    void snap(int j) {
        const int reach = WA_TTS_RATE / 8, n_smp = (int) energy.size();
        int s_lo = to_sample(lo[j]), s_hi = to_sample(hi[j]);
        const int w_lo = std::max(s_lo - reach, 0), w_hi = std::min(s_hi + reach, n_smp);
        float total = 0.0f;
        for (int k = w_lo; k < w_hi; ++k) total += energy_at(k);
        const float level = 0.5 * total / (w_hi - w_lo);
        const auto loud = [&](int k) { return energy_at(k) > level; };
        const auto quiet = [&](int k) { return energy_at(k) < level; };
        int k = s_lo;
        if (loud(k) && j > 0) {
            while (k > 0 && loud(k)) --k;
            lo[j] = to_time(k);
            if (lo[j] < hi[j - 1]) lo[j] = hi[j - 1]; else s_lo = k;
        } else {
            while (quiet(k) && k < s_hi) ++k;
            s_lo = k;
            lo[j] = to_time(k);
        }
        k = s_hi;
        if (loud(k)) {
            while (k < n_smp - 1 && loud(k)) ++k;
            hi[j] = to_time(k);
            if (j < n - 1 && hi[j] > lo[j + 1]) hi[j] = lo[j + 1]; else s_hi = k;
        } else {
            while (quiet(k) && k > s_lo) --k;
            s_hi = k;
            hi[j] = to_time(k);
        }
    }
};

// the finalisation's branches, and the record's edge cases: a scan passing s_lo, an inverted window, an empty one (NaN level), level 0
enum { BACK_KEPT, BACK_CLAMPED, LOUD_FIRST, FWD_MOVED, FWD_TO_END, END_KEPT, END_CLAMPED, END_LAST, TRAIL_MOVED, TRAIL_PAST_START, TRAIL_EMPTY, INVERTED, EMPTY, ZERO_LEVEL, B_N };

int main(int argc, char ** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 10000;
    long taken[B_N] = { 0 };
    std::mt19937 rng(20240607);
    auto pick = [&](int a, int b) { return a + (int) (rng() % (unsigned) (b - a + 1)); };
    for (int c = 0; c < cases; ++c) {
        const int n_smp = c % 97 == 0 ? pick(1, 70) : pick(4000, 14000), n = pick(2, 7);
        std::vector<float> e((size_t) n_smp, 0.0f);
        if (c % 53 != 0)                                   // (every 53rd case: silence, level 0)
            for (int at = pick(0, 900); at < n_smp; at += pick(40, 2500)) {
                const float amp = (float) pick(1, 1000) / 1000.0f;
                for (int k = at, end = std::min(n_smp, at + pick(1, 1800)); k < end; ++k) e[(size_t) k] = amp * (float) pick(0, 1000) / 1000.0f;
            }
        const int64_t seg_lo = pick(0, 3000), span = n_smp / 160 + 2;
        old_timeline was = { n, seg_lo, std::vector<int64_t>(n), std::vector<int64_t>(n), e };
        int64_t t = seg_lo - pick(0, 2);
        for (int j = 0; j < n; ++j) {
            was.lo[j] = t;
            t += pick(0, (int) (2 * span / n));
            was.hi[j] = t;
            if (pick(0, 9) == 0) was.lo[j] = was.hi[j] + (pick(0, 2) == 0 ? 25 : pick(1, 40));      // out of order: 25 units = 4000 samples, the empty window
            if (pick(0, 5) == 0) t -= pick(0, 30);                                                  // overlapping neighbours
        }
        std::vector<int64_t> lo = was.lo, hi = was.hi;
        std::vector<int> text(n), s_lo(n), s_hi(n);
        for (int j = 0; j < n; ++j) { text[j] = pick(0, 7) != 0; s_lo[j] = was.to_sample(lo[j]); s_hi[j] = was.to_sample(hi[j]); }
        for (int j = 0; j < n; ++j) if (text[j]) was.snap(j);
        for (int j = 0; j < n; ++j) {
            if (!text[j]) continue;
            const wa_tts_record r = wa_tts_record_host(e.data(), n_smp, s_lo[j], s_hi[j], j > 0);
            const int64_t prev_hi = j > 0 ? hi[j - 1] : 0, next_lo = j < n - 1 ? lo[j + 1] : 0;
            wa_tts_finalise(r, s_lo[j], s_hi[j], seg_lo, j > 0, prev_hi, j < n - 1, next_lo, lo[j], hi[j]);
            if (lo[j] != was.lo[j] || hi[j] != was.hi[j]) {
                fprintf(stderr, "case %d token %d: [%lld, %lld] now, [%lld, %lld] before\n", c, j, (long long) lo[j], (long long) hi[j], (long long) was.lo[j], (long long) was.hi[j]);
                return 1;
            }
            const bool loud_lo = r.flags & WA_TTS_LOUD_LO, loud_hi = r.flags & WA_TTS_LOUD_HI;
            const int w = std::min(s_hi[j] + WA_TTS_REACH, n_smp) - std::max(s_lo[j] - WA_TTS_REACH, 0);
            int final_lo = r.fwd_lo;
            if (loud_lo && j > 0) { const bool clamped = was.to_time(r.back_lo) < prev_hi; taken[clamped ? BACK_CLAMPED : BACK_KEPT]++; final_lo = clamped ? s_lo[j] : r.back_lo; }
            else if (loud_lo) taken[LOUD_FIRST]++;
            else if (r.fwd_lo > s_lo[j]) taken[r.fwd_lo == s_hi[j] ? FWD_TO_END : FWD_MOVED]++;
            if (loud_hi) taken[j < n - 1 && was.to_time(r.fwd_hi) > next_lo ? END_CLAMPED : r.fwd_hi == n_smp - 1 ? END_LAST : END_KEPT]++;
            else if (s_hi[j] <= final_lo) taken[TRAIL_EMPTY]++;
            else if (r.back_hi < s_hi[j]) taken[TRAIL_MOVED]++;
            if (!loud_hi && r.back_hi < s_lo[j]) taken[TRAIL_PAST_START]++;
            if (w < 0) taken[INVERTED]++; else if (w == 0) taken[EMPTY]++; else if (r.level == 0.0f) taken[ZERO_LEVEL]++;
        }
    }
    int missing = 0;
    for (int b = 0; b < B_N; ++b) { printf("branch %d: %ld\n", b, taken[b]); missing += taken[b] == 0; }
    if (missing) fprintf(stderr, "%d branches were never taken\n", missing);
    return missing ? 2 : 0;
}

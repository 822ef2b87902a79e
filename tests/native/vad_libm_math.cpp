// vad_libm_math.cpp - CPU harness of tests/test_vad_libm_math.py: wa_libm.h's tanhf and expf against this process's libm, bit for bit.
//   g++ -O2 -std=c++17 -ffp-contract=off -pthread vad_libm_math.cpp -lm
// One line per sweep (F32 bit patterns lo .. hi of one sign at a stride, at most 16 threads): "<name> <arguments> <mismatches> <first bad, hex>".
#include "../../whisper-rust_amd/csrc/wa_libm.h"

#include <algorithm>
#include <cstdio>
#include <thread>

static const unsigned long long TAB[32] = WA_LIBM_EXP2F_TABLE;

static bool same(float a, float b) { return wa_libm_bits(a) == wa_libm_bits(b) || (a != a && b != b); }
static bool tanh_ok(uint32_t u) { const float x = wa_libm_float(u); return same(tanhf(x), wa_tanhf_libm(x)); }
static bool exp_ok(uint32_t u)  { const float x = wa_libm_float(u); return same(expf(x), wa_expf_full(x, TAB)); }

static void sweep(const char * name, bool (*ok)(uint32_t), uint32_t lo, uint32_t hi, uint32_t stride, uint32_t sign) {
    const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const uint64_t n = ((uint64_t) hi - lo) / stride + 1;
    std::vector<uint64_t> bad(nt, 0), first(nt, ~0ull);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t] {
            for (uint64_t i = n * t / nt; i < n * (t + 1) / nt; ++i) {
                const uint32_t u = (uint32_t) (lo + i * stride) | sign;
                if (!ok(u)) { ++bad[t]; first[t] = std::min<uint64_t>(first[t], u); }
            }
        });
    uint64_t b = 0, f = ~0ull;
    for (unsigned t = 0; t < nt; ++t) { th[t].join(); b += bad[t]; f = std::min(f, first[t]); }
    printf("%s %llu %llu %08llx\n", name, (unsigned long long) n, (unsigned long long) b, (unsigned long long) (b ? f : 0));
}

int main() {
    const uint32_t NEG = 0x80000000u;
    // tanhf: every positive F32 from 2^-60 to 23; negatives at stride 61 (a prime: no binade pattern repeats); the special values one by one
    sweep("tanhf_pos", tanh_ok, 0x21800000u, 0x41b80000u, 1, 0);
    sweep("tanhf_neg", tanh_ok, 0x21800000u, 0x41b80000u, 61, NEG);
    // expf: every F32 of [-104, 89] from 2^-30 up in magnitude (below it the result is 1 or its neighbour: stride 61 down to the subnormals)
    sweep("expf_pos", exp_ok, 0x30800000u, 0x42b20000u, 1, 0);
    sweep("expf_neg", exp_ok, 0x30800000u, 0x42d00000u, 1, NEG);
    sweep("expf_pos_small", exp_ok, 0x00000000u, 0x30800000u, 61, 0);
    sweep("expf_neg_small", exp_ok, 0x00000000u, 0x30800000u, 61, NEG);
    uint64_t bad_t = 0, bad_e = 0, lacking = 0;
    for (uint32_t s : { 0x00000000u, 0x00000001u, 0x007fffffu, 0x00800000u, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u })
        for (uint32_t sign : { 0u, NEG }) { bad_t += !tanh_ok(s | sign); bad_e += !exp_ok(s | sign); }
    printf("tanhf_special 14 %llu 0\nexpf_special 14 %llu 0\n", (unsigned long long) bad_t, (unsigned long long) bad_e);
    // the guard: its probe set holds every edge +-1 ulp with both signs, has its stated size, and passes here
    const std::vector<uint32_t> probe = wa_libm_probe_set();
    for (int i = 0; i < WA_LIBM_N_EDGES; ++i)
        for (int d = -1; d <= 1; ++d) {
            const uint32_t a = WA_LIBM_EDGES[i] + (uint32_t) d;
            if ((WA_LIBM_EDGES[i] == 0 && d < 0) || a > 0x7f800000u) continue;
            for (uint32_t sign : { 0u, NEG }) lacking += std::find(probe.begin(), probe.end(), a | sign) == probe.end();
        }
    printf("edges %d %llu 0\n", WA_LIBM_N_EDGES, (unsigned long long) lacking);
    uint32_t first_bad = 0;
    const bool ok = wa_libm_matches_host(&first_bad);
    printf("guard %zu %d %08x\n", probe.size(), ok ? 0 : 1, first_bad);
}

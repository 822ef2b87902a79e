// vad_math.cpp - CPU harness of tests/test_vad_math.py and tools/gen_golden_vad.py.
//
// Links whisper-rust_amd/csrc/wa_vad_host.cpp (the product's model parser, LSTM recurrence, segment rules, speech-only audio and time
// mapping) and adds what the product computes on the device: a plain scalar restatement of the front end (reflect pad, STFT,
// magnitude, four Conv1d + bias + ReLU, W_ih x + b_ih) in the reference's order of operations.  That restatement is test code only.
//   g++ -O2 -std=c++17 -mavx2 -mf16c -ffp-contract=off vad_math.cpp ../../whisper-rust_amd/csrc/wa_vad_host.cpp
//
// usage: vad_math <script>; one command per line, one answer line (or file) per command:
//   model <path>                      -> "model ok" | "model fail <reason>"
//   audio <path.f32>                  -> "audio <n>"
//   probs <n_samples>                 -> "probs <n> <u32 hex>..."       (state reset first, as whisper_vad_detect_speech)
//   front <n_samples> <out.f32>       -> "front <n_chunks>"             ([n_chunks][512] gate inputs written raw)
//   segments <n_samples> <6 params>   -> "segments <k> <t0> <t1>..."
//   map <n_samples> <6 params> <out.f32> -> "map <n_filtered> table <k> <p> <o>... sweep <m> <v>..."   (filtered audio written raw;
//                                        sweep = the mapped time of every centisecond 0..m-1, m = filtered length in cs + 2)
#include "../../whisper-rust_amd/csrc/wa_vad.h"

#include <immintrin.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

static inline float h2f(uint16_t h) { return _cvtsh_ss(h); }
static inline uint16_t f2h(float f) { return _cvtss_sh(f, _MM_FROUND_TO_NEAREST_INT); }

static float tree32(const float * s) {
    float a[8];
    for (int l = 0; l < 8; ++l) a[l] = (s[l] + s[16 + l]) + (s[8 + l] + s[24 + l]);
    const float t0 = a[0] + a[4], t1 = a[1] + a[5], t2 = a[2] + a[6], t3 = a[3] + a[7];
    return (t0 + t1) + (t2 + t3);
}
// ggml_vec_dot_f16: 32 chains, tree, K % 32 leftovers in F64
static float dot_f16(const uint16_t * x, const uint16_t * y, int n) {
    float s[32] = { 0 };
    const int np = n & ~31;
    for (int k = 0; k < np; ++k) s[k & 31] = fmaf(h2f(x[k]), h2f(y[k]), s[k & 31]);
    double sumf = (double) tree32(s);
    for (int k = np; k < n; ++k) sumf += (double) (h2f(x[k]) * h2f(y[k]));
    return (float) sumf;
}
static float dot_f32(const float * x, const float * y, int n) {      // n % 32 == 0
    float s[32] = { 0 };
    for (int k = 0; k < n; ++k) s[k & 31] = fmaf(x[k], y[k], s[k & 31]);
    return tree32(s);
}

// conv_1d = im2col to F16 (row j = ic * 3 + k, zero outside) then dot; in [C_in][L_in] -> out [C_out][L_out], + bias, ReLU
static std::vector<float> conv_relu(const std::vector<float> & in, int cin, int lin, const std::vector<uint16_t> & w, const std::vector<float> & b,
                                    int cout, int stride) {
    const int lout = (lin + 2 - 3) / stride + 1, K = cin * 3;
    std::vector<float> out((size_t) cout * lout);
    std::vector<uint16_t> col(K);
    for (int t = 0; t < lout; ++t) {
        for (int ic = 0; ic < cin; ++ic)
            for (int k = 0; k < 3; ++k) {
                const int i = t * stride + k - 1;
                col[ic * 3 + k] = (i < 0 || i >= lin) ? 0 : f2h(in[(size_t) ic * lin + i]);
            }
        for (int oc = 0; oc < cout; ++oc) {
            const float v = dot_f16(col.data(), w.data() + (size_t) oc * K, K) + b[oc];
            out[(size_t) oc * lout + t] = v > 0.f ? v : 0.f;
        }
    }
    return out;
}

static void front_chunk(const wa_vad_model & m, const float * window /*512*/, float * gate_in /*512*/) {
    float padded[WA_VAD_WINDOW + 2 * WA_VAD_PAD];
    memcpy(padded + WA_VAD_PAD, window, WA_VAD_WINDOW * sizeof(float));
    float * left = padded + WA_VAD_PAD, * right = padded + WA_VAD_PAD + WA_VAD_WINDOW - 1;
    for (int i = 1; i <= WA_VAD_PAD; ++i) { left[-i] = left[i]; right[i] = right[-i]; }
    uint16_t ph[WA_VAD_WINDOW + 2 * WA_VAD_PAD];
    for (int i = 0; i < WA_VAD_WINDOW + 2 * WA_VAD_PAD; ++i) ph[i] = f2h(padded[i]);
    std::vector<float> mag((size_t) WA_VAD_BINS * 4);
    for (int t = 0; t < 4; ++t)
        for (int c = 0; c < WA_VAD_BINS; ++c) {
            const float re = dot_f16(ph + t * WA_VAD_HOP, m.stft.data() + (size_t) c * WA_VAD_NFFT, WA_VAD_NFFT);
            const float im = dot_f16(ph + t * WA_VAD_HOP, m.stft.data() + (size_t) (WA_VAD_BINS + c) * WA_VAD_NFFT, WA_VAD_NFFT);
            const float r2 = re * re, i2 = im * im;
            mag[(size_t) c * 4 + t] = sqrtf(r2 + i2);
        }
    std::vector<float> x = mag;
    int l = 4;
    for (int i = 0; i < 4; ++i) {
        x = conv_relu(x, WA_VAD_ENC_IN[i], l, m.enc_w[i], m.enc_b[i], WA_VAD_ENC_OUT[i], WA_VAD_ENC_STRIDE[i]);
        l = (l + 2 - 3) / WA_VAD_ENC_STRIDE[i] + 1;
    }
    // l == 1: x[128] is time step 0 of the last layer
    for (int r = 0; r < WA_VAD_GATES; ++r) gate_in[r] = dot_f32(m.w_ih.data() + (size_t) r * WA_VAD_HID, x.data(), WA_VAD_HID) + m.b_ih[r];
}

static std::vector<float> front(const wa_vad_model & m, const float * samples, int n) {
    const int nc = wa_vad_n_chunks(n);
    std::vector<float> out((size_t) nc * WA_VAD_GATES);
    for (int i = 0; i < nc; ++i) {
        float window[WA_VAD_WINDOW] = { 0 };
        const int i0 = i * WA_VAD_WINDOW, len = std::min(WA_VAD_WINDOW, n - i0);
        memcpy(window, samples + i0, (size_t) len * sizeof(float));
        front_chunk(m, window, out.data() + (size_t) i * WA_VAD_GATES);
    }
    return out;
}

static std::vector<float> probs_of(const wa_vad_model & m, const float * samples, int n) {
    const std::vector<float> g = front(m, samples, n);
    const int nc = wa_vad_n_chunks(n);
    std::vector<float> p(nc);
    wa_vad_lstm st; st.reset();
    for (int i = 0; i < nc; ++i) p[i] = wa_vad_step(m, st, g.data() + (size_t) i * WA_VAD_GATES);
    return p;
}

static bool write_f32(const std::string & path, const std::vector<float> & v) {
    FILE * f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(float), v.size(), f) == v.size();
    fclose(f);
    return ok;
}

static whisper_vad_params read_params(std::istringstream & ss) {
    whisper_vad_params p;
    ss >> p.threshold >> p.min_speech_duration_ms >> p.min_silence_duration_ms >> p.max_speech_duration_s >> p.speech_pad_ms >> p.samples_overlap;
    return p;
}

int main(int argc, char ** argv) {
    if (argc < 2) { fprintf(stderr, "usage: vad_math <script>\n"); return 2; }
    std::ifstream script(argv[1]);
    if (!script) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    wa_vad_model model; bool have_model = false;
    std::vector<float> audio;
    std::string line;
    while (std::getline(script, line)) {
        std::istringstream ss(line);
        std::string cmd; ss >> cmd;
        if (cmd.empty()) continue;
        if (cmd == "model") {
            std::string path; ss >> path;
            std::ifstream fin(path, std::ios::binary);
            whisper_model_loader loader = {};
            loader.context = &fin;
            loader.read  = [](void * c, void * o, size_t n) -> size_t { auto * f = (std::ifstream *) c; f->read((char *) o, (std::streamsize) n); return (size_t) f->gcount(); };
            loader.eof   = [](void * c) -> bool { return ((std::ifstream *) c)->eof(); };
            loader.close = [](void *) {};
            std::string err;
            model = wa_vad_model();
            const bool opened = (bool) fin;
            have_model = opened && wa_vad_model_load(&loader, model, err);
            if (have_model) printf("model ok\n"); else printf("model fail %s\n", opened ? err.c_str() : "cannot open");
            continue;
        }
        if (cmd == "audio") {
            std::string path; ss >> path;
            std::ifstream fin(path, std::ios::binary | std::ios::ate);
            if (!fin) { printf("audio fail\n"); return 1; }
            const size_t n = (size_t) fin.tellg() / sizeof(float);
            audio.resize(n); fin.seekg(0); fin.read((char *) audio.data(), (std::streamsize) (n * sizeof(float)));
            printf("audio %zu\n", n);
            continue;
        }
        if (!have_model) { printf("%s fail no model\n", cmd.c_str()); return 1; }
        int n = 0; ss >> n;
        if (n < 0 || (size_t) n > audio.size()) { printf("%s fail n_samples\n", cmd.c_str()); return 1; }
        if (cmd == "probs") {
            const std::vector<float> p = probs_of(model, audio.data(), n);
            printf("probs %zu", p.size());
            for (float v : p) { uint32_t u; memcpy(&u, &v, 4); printf(" %08x", u); }
            printf("\n");
        } else if (cmd == "front") {
            std::string out; ss >> out;
            const std::vector<float> g = front(model, audio.data(), n);
            if (!write_f32(out, g)) { printf("front fail write\n"); return 1; }
            printf("front %d\n", wa_vad_n_chunks(n));
        } else if (cmd == "segments" || cmd == "map") {
            const whisper_vad_params vp = read_params(ss);
            const std::vector<float> p = probs_of(model, audio.data(), n);
            const std::vector<wa_vad_seg> segs = wa_vad_segments_from_probs(p.data(), (int) p.size(), model.n_window, vp);
            if (cmd == "segments") {
                printf("segments %zu", segs.size());
                for (const auto & s : segs) printf(" %lld %lld", (long long) s.start, (long long) s.end);
                printf("\n");
            } else {
                std::string out; ss >> out;
                std::vector<float> filtered; std::vector<wa_vad_map_point> table;
                wa_vad_filter_audio(segs, vp.samples_overlap, audio.data(), n, filtered, table);
                if (!write_f32(out, filtered)) { printf("map fail write\n"); return 1; }
                printf("map %zu table %zu", filtered.size(), table.size());
                for (const auto & t : table) printf(" %lld %lld", (long long) t.processed_time, (long long) t.original_time);
                const long long m = (long long) (filtered.size() * 100 / WHISPER_SAMPLE_RATE) + 2;
                printf(" sweep %lld", m);
                for (long long t = 0; t < m; ++t) printf(" %lld", (long long) wa_vad_map_time(t, table));
                printf("\n");
            }
        } else { printf("unknown command %s\n", cmd.c_str()); return 1; }
    }
    return 0;
}

// vad_lstm_ref.cpp - the yardstick of tests/test_vad_lstm_gpu.py: the product's host recurrence (wa_vad_step, wa_vad_host.cpp) over gate inputs
// and a state the caller supplies (g++ -O2 -mavx2 -mf16c -ffp-contract=off -shared -fPIC, with wa_vad_host.cpp).
#include "../../whisper-rust_amd/csrc/wa_vad.h"

#include <cstring>
#include <fstream>

// n rows of gates [n][512]; h, c [128] are read, advanced and written back; probs [n].  0, or -1 where the model file is refused
extern "C" int vad_lstm_ref(const char * model_path, const float * gates, int n, float * h, float * c, float * probs) {
    std::ifstream fin(model_path, std::ios::binary);
    if (!fin) return -1;
    whisper_model_loader loader = {};
    loader.context = &fin;
    loader.read  = [](void * x, void * o, size_t k) -> size_t { auto * f = (std::ifstream *) x; f->read((char *) o, (std::streamsize) k); return (size_t) f->gcount(); };
    loader.eof   = [](void * x) -> bool { return ((std::ifstream *) x)->eof(); };
    loader.close = [](void *) {};
    wa_vad_model m; std::string err;
    if (!wa_vad_model_load(&loader, m, err)) return -1;
    wa_vad_lstm st;
    memcpy(st.h, h, sizeof(st.h)); memcpy(st.c, c, sizeof(st.c));
    for (int i = 0; i < n; ++i) probs[i] = wa_vad_step(m, st, gates + (size_t) i * WA_VAD_GATES);
    memcpy(h, st.h, sizeof(st.h)); memcpy(c, st.c, sizeof(st.c));
    return 0;
}

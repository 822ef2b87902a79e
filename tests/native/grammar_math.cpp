// grammar_math.cpp - drives csrc/wa_grammar.cpp (compiled alone, no HIP) for tests/test_grammar_math.py.
//
// Reads one script (argv[1]) of whitespace-separated words:
//     grammar <n_rules> <i_start_rule>   then per rule:  <n_elements> <type> <value> ...      (the closing END is added here; -1 = a null rule pointer)
//     vocab <n>                          then n token texts in hex ("-" = empty text)
//     cases <n>                          then per case:  <n_tokens> <hex> ...                  (token texts accepted one after the other)
// Prints "refused <reason>" and stops, or "ok" and per case one line: <n_stacks> <n_remain> <n_rejected> <id> ...
// Every case is answered twice, by a fresh cache and by the cache that served the cases before it; the two must agree.
#include "../../whisper-rust_amd/csrc/wa_grammar.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

static std::string unhex(const std::string & h) {
    std::string s;
    if (h == "-") return s;
    for (size_t i = 0; i + 1 < h.size(); i += 2) s.push_back((char) strtol(h.substr(i, 2).c_str(), nullptr, 16));
    return s;
}

int main(int argc, char ** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s script\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    std::string word;
    size_t n_rules = 0, i_start = 0;
    if (!(in >> word >> n_rules >> i_start) || word != "grammar") { fprintf(stderr, "bad script\n"); return 2; }
    std::vector<std::vector<whisper_grammar_element>> rules(n_rules);
    std::vector<char> is_null(n_rules, 0);
    for (size_t i = 0; i < n_rules; ++i) {
        auto & r = rules[i];
        long n = 0; in >> n;
        if (n < 0) { is_null[i] = 1; continue; }
        for (long k = 0; k < n; ++k) { int t; unsigned long v; in >> t >> v; r.push_back({ (whisper_gretype) t, (uint32_t) v }); }
        r.push_back({ WHISPER_GRETYPE_END, 0 });
    }
    std::vector<const whisper_grammar_element *> ptrs;
    for (size_t i = 0; i < n_rules; ++i) ptrs.push_back(is_null[i] ? nullptr : rules[i].data());

    wa_grammar_rules g;
    if (const char * why = wa_grammar_build(g, ptrs.data(), n_rules, i_start)) { printf("refused %s\n", why); return 0; }
    printf("ok\n");

    size_t n_vocab = 0;
    in >> word >> n_vocab;
    std::vector<std::string> vocab(n_vocab);
    for (auto & t : vocab) { in >> word; t = unhex(word); }
    wa_grammar_vocab v;
    wa_grammar_vocab_build(v, vocab, (int) n_vocab);

    size_t n_cases = 0;
    in >> word >> n_cases;
    wa_grammar_cache shared;
    for (size_t c = 0; c < n_cases; ++c) {
        size_t n_tok = 0; in >> n_tok;
        wa_grammar_state s;
        wa_grammar_init(g, s);
        for (size_t k = 0; k < n_tok; ++k) { in >> word; wa_grammar_accept(g, s, unhex(word).c_str()); }
        wa_grammar_cache fresh;
        const std::vector<int32_t> a = wa_grammar_rejects(g, v, s, fresh);
        const std::vector<int32_t> b = wa_grammar_rejects(g, v, s, shared);
        const std::vector<int32_t> b2 = wa_grammar_rejects(g, v, s, shared);      // (the second time from the kept result)
        if (a != b || a != b2) { printf("cache mismatch in case %zu\n", c); return 1; }
        printf("%zu %d %zu", s.stacks.size(), s.partial.n_remain, a.size());
        for (int32_t id : a) printf(" %d", id);
        printf("\n");
    }
    return 0;
}

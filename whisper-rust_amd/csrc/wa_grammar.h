// wa_grammar.h - grammar-constrained sampling (whisper_full_params::grammar_rules): the host-side rule between two decoder passes.
//
// Behavioural contract: sys/whisper.cpp/src/whisper.cpp:5479-5893.  It is a contract of SETS - which token ids of the vocabulary no
// pushdown stack of a decoder accepts - so the structure here is our own:
//   wa_grammar_rules  one immutable table per whisper_full call: every rule back to back, validated once.  A stack is a vector of
//                     element positions in that table (the reference keeps raw pointers into the caller's arrays and into other
//                     decoders' copies of the rules; every copy holds the same content, positions name it once).
//   wa_grammar_vocab  the code points of every candidate token (id < eot, non-empty text) decoded once per context from a clean
//                     partial state; tokens are re-decoded only while a decoder carries a partial UTF-8 sequence.
//   wa_grammar_state  per decoder: the set of stacks (sorted, duplicates removed: acceptance is a property of the set) + the partial
//                     sequence.  This is what a beam candidate snapshots.
//   wa_grammar_cache  per decoder, never copied with the state: stack sets seen in this call, their transitions per code point and
//                     the rejected ids of each set.  A grammar visits few distinct sets, so most steps are one look-up.
// Plain C++ (no HIP, no device types): tests/native/grammar_math.cpp compiles this file alone.
#pragma once

#include "../../include/whisper_amd.h"

#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

// returned by whisper_full* for a grammar that the reference would abort on or recurse through without end
#define WA_ERR_GRAMMAR (-20)

struct wa_partial_utf8 { uint32_t value = 0; int n_remain = 0; };     // whisper.cpp: whisper_partial_utf8; n_remain -1 = invalid sequence

struct wa_grammar_rules {
    std::vector<whisper_grammar_element> el;    // every rule, each closed by an END element
    std::vector<uint32_t> rule_at;              // position of rule r's first element
    uint32_t start = 0;                         // i_start_rule
    bool empty() const { return rule_at.empty(); }
};

typedef std::vector<uint32_t> wa_gstack;        // element positions, top of the stack last; empty = derivation complete

struct wa_grammar_state {
    std::vector<wa_gstack> stacks;              // no stack at all: the grammar is off for this decoder until the next wa_grammar_init
    wa_partial_utf8 partial;
};

struct wa_grammar_vocab {
    const std::vector<std::string> * text = nullptr;
    int n_ids = 0;                              // ids [0, n_ids) are candidates if their text is not empty
    std::vector<uint32_t> at;                   // [n_ids + 1]: code points of id i are cp[at[i] .. at[i + 1])
    std::vector<uint32_t> cp;
    std::vector<wa_partial_utf8> tail;          // what the token ends in
};

struct wa_grammar_cache {
    std::map<std::vector<wa_gstack>, int> id_of;
    std::vector<const std::vector<wa_gstack> *> sets;       // (keys of id_of: map nodes do not move)
    std::unordered_map<uint64_t, int> next;                 // (set << 32 | code point) -> set, -1: no stack survives
    std::map<int, std::vector<int32_t>> rejects;            // per set, clean partial state
    size_t n_rejected = 0;                                  // ids held by `rejects` in all
    std::vector<int32_t> scratch;
    std::vector<uint32_t> cp_scratch;
    void clear() { id_of.clear(); sets.clear(); next.clear(); rejects.clear(); n_rejected = 0; }
    void release() { *this = wa_grammar_cache(); }          // clear() and give the memory back
};
// What one decoder's cache may hold before it starts over (checked at the start of every wa_grammar_rejects; one scan of the vocabulary adds at
// most one transition per code point of its texts): 4 M rejected ids = 16 MB, 1 M transitions, 4096 sets.
#define WA_GRAMMAR_CACHE_MAX_REJECTED (4u << 20)
#define WA_GRAMMAR_CACHE_MAX_NEXT     (1u << 20)
#define WA_GRAMMAR_CACHE_MAX_SETS     4096u

// Copies and validates the caller's rules.  Returns nullptr, or the reason the grammar is refused: a start rule or a RULE_REF outside the
// table, a null rule, an unknown element type, CHAR_RNG_UPPER / CHAR_ALT that do not continue a char element, a rule that reaches itself
// leftmost without consuming a character (in any rule of the table, reachable from the start rule or not).
const char * wa_grammar_build(wa_grammar_rules & g, const whisper_grammar_element * const * rules, size_t n_rules, size_t i_start_rule);

// Decodes `src` up to its first NUL, continuing `start`; appends the complete code points to `out` (none for an invalid sequence).
wa_partial_utf8 wa_utf8_decode(const char * src, wa_partial_utf8 start, std::vector<uint32_t> & out);

void wa_grammar_vocab_build(wa_grammar_vocab & v, const std::vector<std::string> & id_to_token, int n_ids);

void wa_grammar_init(const wa_grammar_rules & g, wa_grammar_state & s);        // one stack per alternate of the start rule, advanced

// The ids that no stack of `s` accepts, ascending.  Nothing when `s` has no stack.  The reference stays valid until the next call on `c`.
const std::vector<int32_t> & wa_grammar_rejects(const wa_grammar_rules & g, const wa_grammar_vocab & v, const wa_grammar_state & s, wa_grammar_cache & c);

// A sampled token: text that begins with "[_" (timestamps, EOT, the other specials) is skipped; every complete code point advances the
// stacks, stacks that do not match drop out; the partial state is replaced.
void wa_grammar_accept(const wa_grammar_rules & g, wa_grammar_state & s, const char * text);

// wa_grammar.cpp - see wa_grammar.h.  Every rule cites the reference lines it reproduces (sys/whisper.cpp/src/whisper.cpp).
#include "wa_grammar.h"

#include <algorithm>

namespace {

inline bool ends_sequence(const whisper_grammar_element & e) { return e.type == WHISPER_GRETYPE_END || e.type == WHISPER_GRETYPE_ALT; }    // :5541
inline bool is_char(const whisper_grammar_element & e) { return e.type == WHISPER_GRETYPE_CHAR || e.type == WHISPER_GRETYPE_CHAR_NOT; }

// does `chr` satisfy the char element at `pos`; *after = the position behind the element (:5551-5573)
bool match_char(const wa_grammar_rules & g, uint32_t pos, uint32_t chr, uint32_t * after) {
    const auto * el = g.el.data();
    const bool positive = el[pos].type == WHISPER_GRETYPE_CHAR;
    bool found = false;
    do {
        if (el[pos + 1].type == WHISPER_GRETYPE_CHAR_RNG_UPPER) { found = found || (el[pos].value <= chr && chr <= el[pos + 1].value); pos += 2; }
        else { found = found || el[pos].value == chr; pos += 1; }
    } while (el[pos].type == WHISPER_GRETYPE_CHAR_ALT);
    if (after) *after = pos;
    return found == positive;
}

// could some completion of the partial sequence satisfy the char element at `pos` (:5578-5622): a range-overlap test
bool match_partial(const wa_grammar_rules & g, uint32_t pos, wa_partial_utf8 partial) {
    const auto * el = g.el.data();
    const bool positive = el[pos].type == WHISPER_GRETYPE_CHAR;
    const int n_remain = partial.n_remain;
    if (n_remain < 0 || (n_remain == 1 && partial.value < 2)) return false;       // invalid, or a 7-bit char spread over two bytes (overlong)
    uint32_t low = partial.value << (n_remain * 6);
    const uint32_t high = low | ((1u << (n_remain * 6)) - 1);
    if (low == 0) {
        if (n_remain == 2) low = 1u << 11;
        else if (n_remain == 3) low = 1u << 16;
    }
    do {
        if (el[pos + 1].type == WHISPER_GRETYPE_CHAR_RNG_UPPER) { if (el[pos].value <= high && low <= el[pos + 1].value) return positive; pos += 2; }
        else { if (low <= el[pos].value && el[pos].value <= high) return positive; pos += 1; }
    } while (el[pos].type == WHISPER_GRETYPE_CHAR_ALT);
    return !positive;
}

// A stack whose top may be a RULE_REF becomes the stacks it stands for, each with a char element on top or empty (:5625-5678).  The
// reference recurses; a work list does the same without depending on the depth of the grammar (validation guarantees that it ends).
void advance(const wa_grammar_rules & g, wa_gstack stack, std::vector<wa_gstack> & out) {
    std::vector<wa_gstack> work;
    work.push_back(std::move(stack));
    while (!work.empty()) {
        wa_gstack cur = std::move(work.back());
        work.pop_back();
        if (cur.empty() || is_char(g.el[cur.back()])) { out.push_back(std::move(cur)); continue; }
        const uint32_t pos = cur.back();            // a RULE_REF: replaced by each alternate of its rule, the element behind it kept below
        cur.pop_back();
        if (!ends_sequence(g.el[pos + 1])) cur.push_back(pos + 1);
        for (uint32_t sub = g.rule_at[g.el[pos].value];;) {
            wa_gstack alt = cur;
            if (!ends_sequence(g.el[sub])) alt.push_back(sub);
            work.push_back(std::move(alt));
            while (!ends_sequence(g.el[sub])) ++sub;
            if (g.el[sub].type != WHISPER_GRETYPE_ALT) break;
            ++sub;
        }
    }
}

void canonical(std::vector<wa_gstack> & stacks) {
    std::sort(stacks.begin(), stacks.end());
    stacks.erase(std::unique(stacks.begin(), stacks.end()), stacks.end());
}

// the stacks that remain after code point `chr` (:5684-5710)
std::vector<wa_gstack> accept_char(const wa_grammar_rules & g, const std::vector<wa_gstack> & stacks, uint32_t chr) {
    std::vector<wa_gstack> out;
    for (const auto & st : stacks) {
        if (st.empty()) continue;
        uint32_t after;
        if (!match_char(g, st.back(), chr, &after)) continue;
        wa_gstack nst(st.begin(), st.end() - 1);
        if (!ends_sequence(g.el[after])) nst.push_back(after);
        advance(g, std::move(nst), out);
    }
    canonical(out);
    return out;
}

int intern(wa_grammar_cache & c, std::vector<wa_gstack> && set) {
    if (set.empty()) return -1;
    auto it = c.id_of.find(set);
    if (it != c.id_of.end()) return it->second;
    const int id = (int) c.sets.size();
    it = c.id_of.emplace(std::move(set), id).first;
    c.sets.push_back(&it->first);
    return id;
}

int step(const wa_grammar_rules & g, wa_grammar_cache & c, int set, uint32_t chr) {
    const uint64_t key = ((uint64_t) (uint32_t) set << 32) | chr;
    auto it = c.next.find(key);
    if (it != c.next.end()) return it->second;
    const int to = intern(c, accept_char(g, *c.sets[set], chr));
    c.next.emplace(key, to);
    return to;
}

// One token against the SET of stacks (:5712-5782: rejected by the set = rejected along every path).  Its code points are walked up to the
// first zero (the reference's candidates are zero-terminated arrays); an empty stack takes no further code point and no trailing partial.
bool rejected(const wa_grammar_rules & g, wa_grammar_cache & c, int set, const uint32_t * cp, const uint32_t * end, wa_partial_utf8 tail) {
    for (; cp != end && *cp != 0; ++cp) {
        set = step(g, c, set, *cp);
        if (set < 0) return true;
    }
    if (tail.n_remain == 0) return false;
    for (const auto & st : *c.sets[set]) if (!st.empty() && match_partial(g, st.back(), tail)) return false;
    return true;
}

} // namespace

const char * wa_grammar_build(wa_grammar_rules & g, const whisper_grammar_element * const * rules, size_t n_rules, size_t i_start_rule) {
    g.el.clear(); g.rule_at.clear(); g.start = 0;
    if (i_start_rule >= n_rules) return "i_start_rule is not a rule of the grammar";
    for (size_t r = 0; r < n_rules; ++r) {
        if (!rules[r]) { g.rule_at.clear(); return "a rule pointer is null"; }
        g.rule_at.push_back((uint32_t) g.el.size());
        const whisper_grammar_element * e = rules[r];
        for (; e->type != WHISPER_GRETYPE_END; ++e) g.el.push_back(*e);
        g.el.push_back({ WHISPER_GRETYPE_END, 0 });
    }
    g.start = (uint32_t) i_start_rule;
    const char * why = nullptr;
    for (size_t i = 0; i < g.el.size() && !why; ++i) {
        const auto & e = g.el[i];
        const int prev = i > 0 ? (int) g.el[i - 1].type : (int) WHISPER_GRETYPE_END;
        const bool in_char = prev == WHISPER_GRETYPE_CHAR || prev == WHISPER_GRETYPE_CHAR_NOT || prev == WHISPER_GRETYPE_CHAR_ALT;
        switch ((int) e.type) {
            case WHISPER_GRETYPE_END: case WHISPER_GRETYPE_ALT: case WHISPER_GRETYPE_CHAR: case WHISPER_GRETYPE_CHAR_NOT: break;
            case WHISPER_GRETYPE_RULE_REF: if (e.value >= n_rules) why = "a RULE_REF names a rule that the grammar does not have"; break;
            case WHISPER_GRETYPE_CHAR_RNG_UPPER: if (!in_char) why = "a CHAR_RNG_UPPER does not follow a char element"; break;
            case WHISPER_GRETYPE_CHAR_ALT: if (!in_char && prev != WHISPER_GRETYPE_CHAR_RNG_UPPER) why = "a CHAR_ALT does not follow a char element"; break;
            default: why = "unknown element type";
        }
    }
    if (!why) {
        // Left recursion: the reference expands a RULE_REF on top of a stack before any character is consumed, so a rule that reaches itself
        // through leftmost references - behind references that can derive nothing, too - never stops expanding.
        const size_t n = n_rules;
        std::vector<char> nullable(n, 0);
        for (bool changed = true; changed;) {
            changed = false;
            for (size_t r = 0; r < n; ++r) {
                if (nullable[r]) continue;
                bool all = true;            // of the alternate being scanned: only nullable references so far
                for (uint32_t i = g.rule_at[r];; ++i) {
                    const auto & e = g.el[i];
                    if (ends_sequence(e)) {
                        if (all) { nullable[r] = 1; changed = true; break; }
                        if (e.type == WHISPER_GRETYPE_END) break;
                        all = true;
                    } else if (!(e.type == WHISPER_GRETYPE_RULE_REF && nullable[e.value])) all = false;
                }
            }
        }
        std::vector<std::vector<uint32_t>> left(n);     // r -> the rules it can have on top without consuming a character
        for (size_t r = 0; r < n; ++r) {
            bool open = true;
            for (uint32_t i = g.rule_at[r];; ++i) {
                const auto & e = g.el[i];
                if (e.type == WHISPER_GRETYPE_END) break;
                if (e.type == WHISPER_GRETYPE_ALT) { open = true; continue; }
                if (!open) continue;
                if (e.type == WHISPER_GRETYPE_RULE_REF) { left[r].push_back(e.value); open = nullable[e.value] != 0; }
                else open = false;
            }
        }
        std::vector<char> colour(n, 0);                 // 0 new, 1 on the path, 2 done
        std::vector<std::pair<uint32_t, size_t>> path;
        for (size_t r0 = 0; r0 < n && !why; ++r0) {
            if (colour[r0]) continue;
            path.push_back({ (uint32_t) r0, 0 }); colour[r0] = 1;
            while (!path.empty() && !why) {
                auto & top = path.back();
                if (top.second == left[top.first].size()) { colour[top.first] = 2; path.pop_back(); continue; }
                const uint32_t q = left[top.first][top.second++];
                if (colour[q] == 1) why = "a rule reaches itself leftmost without consuming a character (left recursion)";
                else if (colour[q] == 0) { colour[q] = 1; path.push_back({ q, 0 }); }
            }
        }
    }
    if (why) { g.el.clear(); g.rule_at.clear(); g.start = 0; }
    return why;
}

wa_partial_utf8 wa_utf8_decode(const char * src, wa_partial_utf8 start, std::vector<uint32_t> & out) {    // :5484-5538
    static const int lookup[] = { 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 2, 2, 3, 4 };
    const size_t out0 = out.size();
    const unsigned char * pos = (const unsigned char *) src;
    uint32_t value = start.value;
    int n_remain = start.n_remain;
    while (*pos != 0 && n_remain > 0) {             // the carried sequence goes on: only continuation bytes may follow
        if ((*pos >> 6) != 2) { out.resize(out0); return { 0, -1 }; }
        value = (value << 6) + (*pos & 0x3F);
        ++pos; --n_remain;
    }
    if (start.n_remain > 0 && n_remain == 0) out.push_back(value);
    while (*pos != 0) {
        n_remain = lookup[*pos >> 4] - 1;
        if (n_remain < 0) { out.resize(out0); return { 0, -1 }; }       // a continuation byte where a sequence starts
        const uint8_t mask = (uint8_t) ((1 << (7 - n_remain)) - 1);
        value = *pos & mask;
        ++pos;
        while (*pos != 0 && n_remain > 0) {         // (as the reference: the bytes inside a sequence are taken as they come)
            value = (value << 6) + (*pos & 0x3F);
            ++pos; --n_remain;
        }
        if (n_remain == 0) out.push_back(value);
    }
    return { value, n_remain };
}

void wa_grammar_vocab_build(wa_grammar_vocab & v, const std::vector<std::string> & id_to_token, int n_ids) {
    v.text = &id_to_token;
    v.n_ids = std::max(0, std::min(n_ids, (int) id_to_token.size()));
    v.at.assign((size_t) v.n_ids + 1, 0);
    v.cp.clear();
    v.tail.assign((size_t) v.n_ids, wa_partial_utf8());
    for (int i = 0; i < v.n_ids; ++i) {
        v.at[i] = (uint32_t) v.cp.size();
        if (!id_to_token[i].empty()) v.tail[i] = wa_utf8_decode(id_to_token[i].c_str(), wa_partial_utf8(), v.cp);
    }
    v.at[v.n_ids] = (uint32_t) v.cp.size();
}

void wa_grammar_init(const wa_grammar_rules & g, wa_grammar_state & s) {          // :5799-5821
    s.stacks.clear();
    s.partial = wa_partial_utf8();
    if (g.empty()) return;
    for (uint32_t pos = g.rule_at[g.start];;) {
        wa_gstack st;
        if (!ends_sequence(g.el[pos])) st.push_back(pos);
        advance(g, std::move(st), s.stacks);
        while (!ends_sequence(g.el[pos])) ++pos;
        if (g.el[pos].type != WHISPER_GRETYPE_ALT) break;
        ++pos;
    }
    canonical(s.stacks);
}

const std::vector<int32_t> & wa_grammar_rejects(const wa_grammar_rules & g, const wa_grammar_vocab & v, const wa_grammar_state & s, wa_grammar_cache & c) {
    c.scratch.clear();
    if (g.empty() || s.stacks.empty()) return c.scratch;
    // a grammar with many distinct stack sets (unbounded nesting): start over rather than grow without limit
    if (c.sets.size() > WA_GRAMMAR_CACHE_MAX_SETS || c.next.size() > WA_GRAMMAR_CACHE_MAX_NEXT || c.n_rejected > WA_GRAMMAR_CACHE_MAX_REJECTED) c.clear();
    std::vector<wa_gstack> key = s.stacks;
    canonical(key);
    const int set = intern(c, std::move(key));
    const auto & text = *v.text;
    if (s.partial.n_remain == 0) {                  // the common case: the code points decoded once per context, the result kept per set
        auto it = c.rejects.find(set);
        if (it != c.rejects.end()) return it->second;
        std::vector<int32_t> out;
        for (int id = 0; id < v.n_ids; ++id) {
            if (text[id].empty()) continue;
            if (rejected(g, c, set, v.cp.data() + v.at[id], v.cp.data() + v.at[id + 1], v.tail[id])) out.push_back(id);
        }
        c.n_rejected += out.size();
        return c.rejects.emplace(set, std::move(out)).first->second;
    }
    for (int id = 0; id < v.n_ids; ++id) {          // a partial sequence is pending: every token continues it
        if (text[id].empty()) continue;
        c.cp_scratch.clear();
        const wa_partial_utf8 tail = wa_utf8_decode(text[id].c_str(), s.partial, c.cp_scratch);
        if (rejected(g, c, set, c.cp_scratch.data(), c.cp_scratch.data() + c.cp_scratch.size(), tail)) c.scratch.push_back(id);
    }
    return c.scratch;
}

void wa_grammar_accept(const wa_grammar_rules & g, wa_grammar_state & s, const char * text) {            // :5868-5890
    if (g.empty() || s.stacks.empty()) return;
    if (text[0] == '[' && text[1] == '_') return;
    std::vector<uint32_t> cps;
    const wa_partial_utf8 tail = wa_utf8_decode(text, s.partial, cps);
    for (uint32_t chr : cps) s.stacks = accept_char(g, s.stacks, chr);
    s.partial = tail;
}

"""Grammars for the grammar-constrained decoding tests, as whisper_grammar_element arrays, and a brute-force acceptor.

whisper.h has no GBNF text parser, so the grammars are written the way a caller hands them over: per rule a list of
(type, value) elements without the closing END (the mirror in whisper_rs.py and the native test add it); ALT separates the
alternates of a rule.  GOLDEN names the grammars behind tests/golden/s128_grammar.json.

The acceptor below shares nothing with csrc/wa_grammar.cpp.  It keeps no pushdown stacks: it is a chart recogniser (Earley
items over code points) that answers "is the text so far plus this token still the beginning of a sentence of the
grammar", plus the reference's rule for a token that ends inside a UTF-8 sequence (sys/whisper.cpp/src/whisper.cpp:5578-5622:
the code points the sequence can still complete to must overlap a range of the char element that is expected next; a
negated element accepts only if none of its ranges overlaps).  Test infrastructure only; never imported by the product.
"""
from __future__ import annotations

END, ALT, RULE_REF, CHAR, CHAR_NOT, CHAR_RNG_UPPER, CHAR_ALT = range(7)


def lit(text: str):
    return [(CHAR, ord(c)) for c in text]


def rng(lo: str, hi: str, first: bool = True, negate: bool = False):
    return [((CHAR_NOT if negate else CHAR) if first else CHAR_ALT, ord(lo)), (CHAR_RNG_UPPER, ord(hi))]


# root ::= word root | word ; word ::= " " letters ; letters ::= [a-m] letters | [a-m]
G_LETTERS = ([
    [(RULE_REF, 1), (RULE_REF, 0), (ALT, 0), (RULE_REF, 1)],
    lit(" ") + [(RULE_REF, 2)],
    rng("a", "m") + [(RULE_REF, 2), (ALT, 0)] + rng("a", "m"),
], 0)

# root ::= " ab " [cd] [e-k] : a finite language; once it is derived every stack is empty and every text token is rejected
G_FINITE = ([
    lit(" ab ") + [(CHAR, ord("c")), (CHAR_ALT, ord("d"))] + rng("e", "k"),
], 0)

# root ::= ch root | ch ; ch ::= [^n-zae] : a negated element with a range and two single alternates
G_NOT = ([
    [(RULE_REF, 1), (RULE_REF, 0), (ALT, 0), (RULE_REF, 1)],
    [(CHAR_NOT, ord("n")), (CHAR_RNG_UPPER, ord("z")), (CHAR_ALT, ord("a")), (CHAR_ALT, ord("e"))],
], 0)

# root ::= [\x80-\U0010FFFF] root | [\x80-\U0010FFFF] : only multi-byte characters (the s128u vocabulary)
G_NONASCII = ([
    [(CHAR, 0x80), (CHAR_RNG_UPPER, 0x10FFFF), (RULE_REF, 0), (ALT, 0), (CHAR, 0x80), (CHAR_RNG_UPPER, 0x10FFFF)],
], 0)

# vowel ::= [aeiou] ; cons ::= [b-df-hj-np-tv-z] ; start ::= sp cons vowel start | sp vowel cons start | sp cons vowel | sp vowel ; sp ::= " " |
# several rules, four alternates in the start rule, i_start_rule = 2, and a reference that can derive nothing in front of each alternate
G_SYLLABLES = ([
    [(CHAR, ord("a")), (CHAR_ALT, ord("e")), (CHAR_ALT, ord("i")), (CHAR_ALT, ord("o")), (CHAR_ALT, ord("u"))],
    rng("b", "d") + rng("f", "h", False) + rng("j", "n", False) + rng("p", "t", False) + rng("v", "z", False),
    [(RULE_REF, 3), (RULE_REF, 1), (RULE_REF, 0), (RULE_REF, 2), (ALT, 0),
     (RULE_REF, 3), (RULE_REF, 0), (RULE_REF, 1), (RULE_REF, 2), (ALT, 0),
     (RULE_REF, 3), (RULE_REF, 1), (RULE_REF, 0), (ALT, 0),
     (RULE_REF, 3), (RULE_REF, 0)],
    lit(" ") + [(ALT, 0)],
], 2)

GOLDEN = {"letters": G_LETTERS, "finite": G_FINITE, "not": G_NOT, "nonascii": G_NONASCII, "syllables": G_SYLLABLES}

# grammars that whisper_full refuses (return code -20): name -> (rules, i_start_rule)
MALFORMED = {
    "start_rule_missing": ([lit("a")], 1),
    "start_rule_missing_of_three": (G_LETTERS[0], 3),
    "rule_pointer_null": ([[(RULE_REF, 1)], None, lit("a")], 0),      # None: a null pointer in the array of rules
    "rule_ref_missing": ([[(RULE_REF, 3)], lit("a")], 0),
    "range_without_char": ([[(CHAR_RNG_UPPER, ord("z"))]], 0),
    "range_after_range": ([rng("a", "c") + [(CHAR_RNG_UPPER, ord("z"))]], 0),
    "alt_char_without_char": ([[(RULE_REF, 1), (CHAR_ALT, ord("b"))], lit("a")], 0),
    "left_recursion_direct": ([[(RULE_REF, 0), (CHAR, ord("x")), (ALT, 0), (CHAR, ord("y"))]], 0),
    "left_recursion_indirect": ([[(RULE_REF, 1), (CHAR, ord("x"))], [(RULE_REF, 2), (ALT, 0), (CHAR, ord("y"))], [(RULE_REF, 0), (CHAR, ord("z"))]], 0),
    # a ::= b a "x" | "y" ; b ::= "z" |   : `a` is leftmost behind a reference that can derive nothing
    "left_recursion_behind_empty": ([[(RULE_REF, 1), (RULE_REF, 0), (CHAR, ord("x")), (ALT, 0), (CHAR, ord("y"))], [(CHAR, ord("z")), (ALT, 0)]], 0),
    # the start rule never reaches the recursive rule: the reference would finish this one; any such rule in the table is refused
    "left_recursion_unreachable": ([lit("a"), [(RULE_REF, 1), (CHAR, ord("x"))]], 0),
    "unknown_element_type": ([[(9, 0)]], 0),
}
# right recursion, recursion behind a consumed character and a reference to an empty rule are fine
WELL_FORMED_EDGE = {
    "right_recursion_behind_char": ([[(CHAR, ord("(")), (RULE_REF, 0), (CHAR, ord(")")), (ALT, 0), (CHAR, ord("x"))]], 0),
    "empty_rule_then_char": ([[(RULE_REF, 1), (CHAR, ord("a")), (RULE_REF, 0), (ALT, 0), (RULE_REF, 1)], []], 0),
}


# --------------------------------------------------------------------------------------------------
# brute-force acceptor
# --------------------------------------------------------------------------------------------------
def utf8_step(data: bytes, value: int, n_remain: int):
    """Code points of `data` (cut at its first NUL) continuing a pending sequence; returns (code points, value, n_remain) with
    n_remain = -1 and no code points for an invalid token.  As the engine: a pending sequence carried in from the previous token
    must continue with continuation bytes; a sequence that starts inside the token takes its next bytes as they come."""
    data = data.split(b"\0")[0]
    cps, i = [], 0
    carried = n_remain > 0
    while i < len(data) and n_remain > 0:
        if data[i] >> 6 != 2:
            return [], 0, -1
        value = ((value << 6) + (data[i] & 0x3F)) & 0xFFFFFFFF
        i += 1
        n_remain -= 1
    if carried and n_remain == 0:
        cps.append(value)
    while i < len(data):
        b = data[i]
        if b < 0x80:
            n_remain, value = 0, b
        elif b < 0xC0:
            return [], 0, -1
        elif b < 0xE0:
            n_remain, value = 1, b & 0x3F
        elif b < 0xF0:
            n_remain, value = 2, b & 0x1F
        else:
            n_remain, value = 3, b & 0x0F
        i += 1
        while i < len(data) and n_remain > 0:
            value = ((value << 6) + (data[i] & 0x3F)) & 0xFFFFFFFF
            i += 1
            n_remain -= 1
        if n_remain == 0:
            cps.append(value)
    return cps, value, n_remain


class Acceptor:
    def __init__(self, rules, i_start: int):
        self.alts = []          # per rule: list of alternates; an alternate = list of ("ref", r) | ("cls", negated, [(lo, hi), ...])
        for rule in rules:
            alts, cur, k = [], [], 0
            while k < len(rule):
                t, v = rule[k]
                if t == ALT:
                    alts.append(cur); cur = []; k += 1
                elif t == RULE_REF:
                    cur.append(("ref", v)); k += 1
                else:
                    assert t in (CHAR, CHAR_NOT), "element %d cannot start a symbol" % t
                    neg, spans = t == CHAR_NOT, []
                    while True:
                        lo = rule[k][1]; k += 1
                        if k < len(rule) and rule[k][0] == CHAR_RNG_UPPER:
                            spans.append((lo, rule[k][1])); k += 1
                        else:
                            spans.append((lo, lo))
                        if not (k < len(rule) and rule[k][0] == CHAR_ALT):
                            break
                    cur.append(("cls", neg, spans))
            alts.append(cur)
            self.alts.append(alts)
        self.nullable = [False] * len(rules)
        changed = True
        while changed:
            changed = False
            for r, alts in enumerate(self.alts):
                if not self.nullable[r] and any(all(s[0] == "ref" and self.nullable[s[1]] for s in a) for a in alts):
                    self.nullable[r] = changed = True
        # boundaries of every range: code points between two neighbouring boundaries behave alike
        cuts = {0}
        for alts in self.alts:
            for a in alts:
                for s in a:
                    if s[0] == "cls":
                        for lo, hi in s[2]:
                            cuts.add(lo); cuts.add(hi + 1)
        self.cuts = sorted(cuts)
        start = frozenset((i_start, b, 0, 0) for b in range(len(self.alts[i_start])))
        self.chart0 = (self._close((), start),)

    def _close(self, chart, items):
        """Earley closure of a new last set `items` behind the sets `chart`."""
        k = len(chart)
        out, work = set(items), list(items)

        def add(it):
            if it not in out:
                out.add(it); work.append(it)
        while work:
            r, a, d, o = work.pop()
            syms = self.alts[r][a]
            if d == len(syms):
                src = out if o == k else chart[o]
                for (r2, a2, d2, o2) in list(src):
                    s2 = self.alts[r2][a2]
                    if d2 < len(s2) and s2[d2] == ("ref", r):
                        add((r2, a2, d2 + 1, o2))
            elif syms[d][0] == "ref":
                q = syms[d][1]
                for b in range(len(self.alts[q])):
                    add((q, b, 0, k))
                if self.nullable[q]:
                    add((r, a, d + 1, o))
        return frozenset(out)

    @staticmethod
    def _in_class(sym, cp):
        return any(lo <= cp <= hi for lo, hi in sym[2]) != sym[1]

    def scan(self, chart, cp):
        """chart + the set after code point cp, or None when nothing can take it."""
        nxt = set()
        for (r, a, d, o) in chart[-1]:
            syms = self.alts[r][a]
            if d < len(syms) and syms[d][0] == "cls" and self._in_class(syms[d], cp):
                nxt.add((r, a, d + 1, o))
        return chart + (self._close(chart, nxt),) if nxt else None

    def partial_ok(self, chart, value, n_remain):
        if n_remain < 0 or (n_remain == 1 and value < 2):
            return False
        low = (value << (6 * n_remain)) & 0xFFFFFFFF
        high = low | ((1 << (6 * n_remain)) - 1)
        if low == 0 and n_remain == 2:
            low = 1 << 11
        if low == 0 and n_remain == 3:
            low = 1 << 16
        for (r, a, d, o) in chart[-1]:
            syms = self.alts[r][a]
            if d < len(syms) and syms[d][0] == "cls":
                overlap = any(lo <= high and low <= hi for lo, hi in syms[d][2])
                if overlap != syms[d][1]:
                    return True
        return False

    def cell(self, cp):
        import bisect
        return bisect.bisect_right(self.cuts, cp) - 1

    def rejected_ids(self, vocab, n_ids, prefix=()):
        """Ids < n_ids with non-empty text that cannot follow the token texts `prefix`; empty once the prefix itself broke the grammar."""
        chart, value, n_remain = self.chart0, 0, 0
        for tok in prefix:
            if tok.startswith(b"[_"):
                continue
            cps, value, n_remain = utf8_step(tok, value, n_remain)
            for cp in cps:
                chart = self.scan(chart, cp)
                if chart is None:
                    return set()
        memo = {(): chart}          # per sequence of range cells (with one representative code point each): the chart, or None

        def walk(cells, cps):
            if cells not in memo:
                before = walk(cells[:-1], cps[:-1])
                memo[cells] = None if before is None else self.scan(before, cps[-1])
            return memo[cells]
        out = set()
        for i in range(n_ids):
            if not vocab[i]:
                continue
            cps, v, nr = utf8_step(vocab[i], value, n_remain)
            if 0 in cps:
                cps = cps[:cps.index(0)]
            end = walk(tuple(self.cell(c) for c in cps), tuple(cps))
            if end is None or (nr != 0 and not self.partial_ok(end, v, nr)):
                out.add(i)
        return out

"""Grammar-constrained sampling, host part (whisper-rust_amd/csrc/wa_grammar.cpp compiled alone by g++: no HIP, no device).

For every golden grammar of tools/wgrammar.py and a list of scripted token prefixes - among them prefixes that end in the middle
of a character, prefixes that break the grammar, specials that are skipped - the set of token ids that the grammar rejects must
EQUAL the set given by the brute-force acceptor of tools/wgrammar.py (a chart recogniser over code points: no stacks, no shared
code), over the whole synthetic ASCII vocabulary and over the multi-byte variant (wsynth.synth_vocab("utf8")).  Malformed grammars
are refused with a reason; nothing may crash or hang.  CPU only."""
import json
import os
import shutil
import subprocess

import pytest

import wgrammar as G
import wsynth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_IDS = wsynth.N_BASE_VOCAB - 1         # token_eot of the multilingual vocabulary: candidates are the ids below it


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("grammar") / "grammar_math")
    src = os.path.join(ROOT, "whisper-rust_amd", "csrc", "wa_grammar.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "native", "grammar_math.cpp"), src, "-o", out])
    return out


@pytest.fixture(scope="module")
def vocabs():
    return {"ascii": wsynth.synth_vocab(), "utf8": wsynth.synth_vocab("utf8")}


def run(exe, tmp_path, rules, i_start, vocab=(), cases=()):
    hx = lambda b: b.hex() if b else "-"
    lines = ["grammar %d %d" % (len(rules), i_start)]
    for r in rules:
        lines.append("-1" if r is None else " ".join([str(len(r))] + ["%d %d" % (t, v) for t, v in r]))
    lines.append("vocab %d" % len(vocab))
    lines.append(" ".join(hx(w) for w in vocab))
    lines.append("cases %d" % len(cases))
    for c in cases:
        lines.append(" ".join([str(len(c))] + [hx(w) for w in c]))
    script = tmp_path / "script.txt"
    script.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(script)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return out.stdout.splitlines()


E4 = "\U0001F600".encode()      # four bytes
H3 = "中".encode()          # three bytes
PREFIXES = {
    "letters": {
        "ascii": [[], [b" "], [b" ab"], [b" ab", b"c", b" k"], [b" ab", b"[_TT_12]", b"m"], [b" ab", b"[_EOT_]"],
                  [b" n"],                                  # breaks the grammar: it is off from here
                  [b" ab", b"  "], [b"a"]],
        "utf8": [[], [b" a"], [b" a", b"\xc3"],             # ends mid-character, and nothing can complete it to [a-m]
                 [b"\xc3\x80"]],
    },
    "finite": {
        "ascii": [[], [b" ab"], [b" ab", b" "], [b" ab", b" ", b"c"], [b" ab", b" ", b"c", b"e"],        # the last one: derivation complete
                  [b" ab", b" ", b"c", b"e", b"e"], [b" ab", b" ", b" d"]],
        "utf8": [[], [b" ab", b" ", b"d", b"k"]],
    },
    "not": {
        "ascii": [[], [b" b"], [b"b", b"c", b" "], [b"n"], [b"bbbb", b"[_BEG_]"]],
        "utf8": [[], [H3], [H3[:1]], [H3[:2]], [E4[:1]], [E4[:2]], [E4[:3]], [b"\xc3"], [b"\xc1"], [b"\xe0"], [b"\xf0"],
                 [b"\x80"],                                 # a continuation byte where a sequence starts: invalid, the stacks stay
                 [b"\xc3", b"a"],                           # a pending sequence continued by a non-continuation byte
                 [E4[:1], E4[1:2], E4[2:3]], [E4[:1], E4[1:2], E4[2:3], E4[3:]]],
    },
    "nonascii": {
        "ascii": [[], [b"a"]],
        "utf8": [[], [H3], [H3[:1]], [H3[:2]], [H3[:2], H3[2:]], [E4[:1]], [E4[:2]], [E4[:3]], [E4[:1], E4[1:3]], [b"\xd3"], [b"\xd3", b"\xa7"],
                 [b"\xc0"], [b"\xc1"], [b"\xe0"], [b"\xf0"], [b"\xf4"], [b"\xff"], [b"\xd3", b"\xd3"], [b"\xa7"], [b"\xc3\x80", b"\xbf\xc3\x80"],
                 [b"\xe0", b"\x80"], [b"\xc3", b"[_TT_1]", b"\x80"]],
    },
    "syllables": {
        "ascii": [[], [b" "], [b" b"], [b" ba"], [b"a"], [b"ab", b" "], [b" ba", b" e"], [b" ba", b" ec", b"di"], [b"bb"], [b" ", b" "]],
        "utf8": [[], [b"ba", b"\xc3"]],
    },
}


@pytest.mark.parametrize("vname", ["ascii", "utf8"])
@pytest.mark.parametrize("gname", sorted(G.GOLDEN))
def test_rejected_sets_equal_brute_force(exe, vocabs, tmp_path, gname, vname):
    rules, i_start = G.GOLDEN[gname]
    vocab = vocabs[vname]
    cases = PREFIXES[gname][vname]
    lines = run(exe, tmp_path, rules, i_start, vocab[:N_IDS], cases)
    assert lines[0] == "ok", lines[0]
    assert len(lines) == 1 + len(cases)
    acc = G.Acceptor(rules, i_start)
    n_nonempty = 0
    for case, line in zip(cases, lines[1:]):
        f = [int(x) for x in line.split()]
        got = set(f[3:])
        assert len(got) == f[2] == len(f) - 3
        want = acc.rejected_ids(vocab, N_IDS, case)
        assert got == want, (gname, vname, case, len(got), len(want), sorted(got ^ want)[:10])
        n_nonempty += len(got) > 0
    assert n_nonempty >= 1          # (the cases do not all end with the grammar off)


def test_grammar_is_off_after_a_violation_and_complete_after_the_last_character(exe, vocabs, tmp_path):
    rules, i_start = G.GOLDEN["finite"]
    vocab = vocabs["ascii"][:N_IDS]
    lines = run(exe, tmp_path, rules, i_start, vocab, [[b" ab", b" ", b"c", b"e"], [b" ab", b" ", b"c", b"e", b"e"], [b" zz"]])
    done, past, broken = ([int(x) for x in l.split()] for l in lines[1:])
    assert done[0] == 1 and done[2] == N_IDS          # one (empty) stack: every text token rejected
    assert past[0] == 0 and past[2] == 0              # a token after the end emptied the set: nothing is penalised any more
    assert broken[0] == 0 and broken[2] == 0


@pytest.mark.parametrize("name", sorted(G.MALFORMED))
def test_malformed_grammar_is_refused(exe, tmp_path, name):
    rules, i_start = G.MALFORMED[name]
    lines = run(exe, tmp_path, rules, i_start)
    assert lines and lines[0].startswith("refused "), (name, lines)


@pytest.mark.parametrize("name", sorted(G.WELL_FORMED_EDGE))
def test_recursion_behind_a_character_is_accepted(exe, vocabs, tmp_path, name):
    rules, i_start = G.WELL_FORMED_EDGE[name]
    vocab = [b"(", b"x", b")", b"((x", b"))", b"a", b"aa", b"b", b"(x)"]
    cases = [[], [b"("], [b"((x"], [b"((x", b"))"], [b"a"], [b"aa", b"a"]]
    lines = run(exe, tmp_path, rules, i_start, vocab, cases)
    assert lines[0] == "ok"
    acc = G.Acceptor(rules, i_start)
    for case, line in zip(cases, lines[1:]):
        assert set(int(x) for x in line.split()[3:]) == acc.rejected_ids(vocab, len(vocab), case), (name, case)


def test_deep_grammar_neither_overflows_nor_hangs(exe, tmp_path):
    """A chain of 20000 rules, each a reference to the next: the reference engine recurses once per rule; validation and the stack advance
    here use work lists.  The same chain closed into a ring is left recursion and is refused."""
    n = 20000
    chain = [[(G.RULE_REF, r + 1)] for r in range(n - 1)] + [G.lit("a")]
    lines = run(exe, tmp_path, chain, 0, [b"a", b"b", b"aa"], [[], [b"a"]])
    assert lines[0] == "ok"
    assert [int(x) for x in lines[1].split()] == [1, 0, 2, 1, 2]
    assert [int(x) for x in lines[2].split()] == [1, 0, 3, 0, 1, 2]
    ring = chain[:-1] + [[(G.RULE_REF, 0)]]
    assert run(exe, tmp_path, ring, 0)[0].startswith("refused ")


@pytest.mark.parametrize("tag", ["letters_greedy", "not_greedy", "syllables_greedy", "finite_greedy", "nonascii_beam5", "nonascii_sampled"])
def test_reference_goldens_obey_the_grammar(exe, vocabs, tmp_path, tag):
    """The reference engine's own tokens (tests/golden/s128_grammar.json, penalty 100) tie the three together: along the first segment
    of a case - the grammar state starts with the window - no sampled text token is in the rejected set, by wa_grammar.cpp and by the
    brute-force acceptor alike."""
    case = json.load(open(os.path.join(ROOT, "tests", "golden", "s128_grammar.json")))["cases"][tag]
    vocab = vocabs["utf8" if case["model"] == "s128u" else "ascii"]
    rules, i_start = G.GOLDEN[case["grammar"]]
    ids = [t for t in case["segments"][0]["ids"] if t < N_IDS][:8]
    texts = [vocab[t] for t in ids]
    cases = [texts[:k] for k in range(len(texts) + 1)]
    lines = run(exe, tmp_path, rules, i_start, vocab[:N_IDS], cases)
    acc = G.Acceptor(rules, i_start)
    for k, line in enumerate(lines[1:]):
        got = set(int(x) for x in line.split()[3:])
        assert got == acc.rejected_ids(vocab, N_IDS, cases[k]), (tag, k)
        assert got, (tag, k)                                    # the grammar is still on
        if k < len(ids):
            assert ids[k] not in got, (tag, k, texts[k])


def test_reference_low_penalty_golden_breaks_the_grammar_where_the_acceptor_says(exe, vocabs, tmp_path):
    """The low-penalty golden: its first segment obeys the grammar for at least 3 text tokens, then holds a token that the grammar rejects;
    behind that token the rejected set is empty - the grammar is off for the rest of the pass."""
    case = json.load(open(os.path.join(ROOT, "tests", "golden", "s128_grammar.json")))["cases"]["letters_low_penalty"]
    assert 2.0 < case["penalty"] < 100.0
    vocab = vocabs["ascii"]
    rules, i_start = G.GOLDEN[case["grammar"]]
    ids = [t for t in case["segments"][0]["ids"] if t < N_IDS]
    acc = G.Acceptor(rules, i_start)
    n_ok = 0
    while n_ok < len(ids) and ids[n_ok] not in acc.rejected_ids(vocab, N_IDS, [vocab[t] for t in ids[:n_ok]]):
        n_ok += 1
    assert 3 <= n_ok < len(ids), n_ok
    texts = [vocab[t] for t in ids]
    lines = run(exe, tmp_path, rules, i_start, vocab[:N_IDS], [texts[:n_ok], texts[:n_ok + 1]])
    before, after = (set(int(x) for x in l.split()[3:]) for l in lines[1:])
    assert ids[n_ok] in before and not after

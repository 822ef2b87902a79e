"""Grammar-constrained decoding through the C ABI (whisper_full_params::grammar_rules / n_grammar_rules / i_start_rule / grammar_penalty).

The goldens (tests/golden/s128_grammar.json, written by tools/gen_golden_grammar.py) are the REFERENCE ENGINE's segments for the grammars of
tools/wgrammar.py on the seeded s128 / s128u / s128-q5_0 models: greedy, the temperature ladder, best_of 5, beam 5 and 8, a finite grammar
whose derivation completes, multi-byte tokens that end inside a UTF-8 sequence, and a low penalty at which a token breaks the grammar.
Every comparison is exact: ids, text, t0 / t1, p, plog.

Which cases reach the partial-sequence rules (a token that is a lone lead byte, then a token that starts with a continuation byte):
nonascii_beam5 (0xC5 then 0xAF, neighbours in one segment) and nonascii_sampled (0xD5 closes a segment, 0x85 opens the next one of the
same window: timestamp tokens lie between them and are skipped by the grammar, the pending sequence is carried across).  nonascii_greedy
decodes whole characters and ends its window on a lone lead byte - this random model repeats itself under the arg-max.
The `_live` cases take as long as the reference engine needs on the host cores (the ladder: 14 s); the product's share is below 0.5 s each."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import wgrammar as G
import wsynth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAOS_LIB = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")
GOLD = json.load(open(os.path.join(GOLDEN, "s128_grammar.json")))
CASES = sorted(GOLD["cases"])
ERR_GRAMMAR = -20           # a malformed grammar


def _segs(st):
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"], tids=s["tids"],
                 p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]]) for s in st.segments()]


def _model_file(name):
    mp = wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)
    assert hashlib.sha256(open(mp, "rb").read()).hexdigest() == GOLD["models"][name], name
    return mp


def _params(wrs, lib, case, **more):
    kw = dict(case["params"])
    fp = wrs.FullParams(lib, kw.pop("strategy", 0), **kw, **more)
    fp.set("grammar", G.GOLDEN[case["grammar"]])
    fp.set("grammar_penalty", case["penalty"])
    return fp


def _pcm():
    return wsynth.synth_audio(GOLD["audio"]["n_samples"], GOLD["audio"]["seed"])


class _Contexts:
    def __init__(self, wrs, lib, **ctx_kw):
        self.wrs, self.lib, self.ctx_kw, self.open = wrs, lib, ctx_kw, {}

    def get(self, name):
        if name not in self.open:
            self.open[name] = self.wrs.WhisperContext.new_with_params(_model_file(name), self.wrs.WhisperContextParameters(self.lib, **self.ctx_kw), lib=self.lib)
        return self.open[name]

    def close(self):
        for c in self.open.values():
            c.free()


@pytest.fixture(scope="module")
def amd(wrs, amd_lib):
    c = _Contexts(wrs, amd_lib)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(wrs, ref_lib):
    c = _Contexts(wrs, ref_lib, use_gpu=False)
    yield c
    c.close()


def _run(ctxs, case, **more):
    st = ctxs.get(case["model"]).create_state()
    st.full(_params(ctxs.wrs, ctxs.lib, case, **more), _pcm())
    out = _segs(st)
    st.free()
    return out


@pytest.mark.parametrize("tag", CASES)
def test_grammar_case_equals_reference_golden(amd, tag):
    case = GOLD["cases"][tag]
    got = _run(amd, case)
    assert got == case["segments"], (tag, [s["text"][:40] for s in got[:2]], [s["text"][:40] for s in case["segments"][:2]])


@pytest.mark.parametrize("tag", CASES)
def test_grammar_case_equals_reference_live(amd, ref, tag):
    """The same arguments handed to both libraries in this process (the golden file is not consulted)."""
    case = GOLD["cases"][tag]
    assert _run(amd, case) == _run(ref, case, n_threads=8), tag


def test_grammar_on_the_stalled_build(wrs):
    """libwhisper_chaos.so (product waves of the one-launch steps stall at random): the plain steps a grammar decodes on give the same tokens."""
    assert os.path.exists(CHAOS_LIB), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    chaos = wrs.load_library(CHAOS_LIB)
    wrs.set_log_callback(chaos, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    ctxs = _Contexts(wrs, chaos)
    for tag in ("syllables_greedy", "letters_beam5"):
        assert _run(ctxs, GOLD["cases"][tag]) == GOLD["cases"][tag]["segments"], tag
    ctxs.close()


def test_full_batch_with_grammar_equals_solo_runs(amd):
    """Four chunks in lock step (whisper_amd_full_batch) under a grammar: each equals its own whisper_full run.  Members send no run-ahead
    requests while a grammar is active - the device would pick tokens by call-constant rules - so every pass is a plain lock-step pass."""
    wrs, case = amd.wrs, GOLD["cases"]["letters_greedy"]
    ctx = amd.get("s128")
    pcms = [wsynth.synth_audio(480000, s) for s in (0, 1, 2, 3)]
    solo = []
    for pcm in pcms:
        st = ctx.create_state()
        st.full(_params(wrs, amd.lib, case), pcm)
        solo.append(_segs(st))
        st.free()
    assert solo[0] == case["segments"]
    states = [ctx.create_state() for _ in pcms]
    wrs.full_batch(ctx, states, _params(wrs, amd.lib, case), pcms)
    for i, st in enumerate(states):
        assert _segs(st) == solo[i], i
        st.free()


def test_no_grammar_state_survives_a_call(amd):
    """A call with a grammar, then calls without one on the SAME state - no rules, rules with n_grammar_rules == 0, n_grammar_rules > 0 with a
    null pointer: each equals the existing unconstrained golden."""
    wrs, lib = amd.wrs, amd.lib
    want = json.load(open(os.path.join(GOLDEN, "s128.json")))["full"]["greedy_tinc0_seed0"]
    st = amd.get("s128").create_state()
    pcm = wsynth.synth_audio(480000, 0)
    st.full(_params(wrs, lib, GOLD["cases"]["letters_beam5"]), pcm)
    assert _segs(st) == GOLD["cases"]["letters_beam5"]["segments"]
    plain = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    st.full(plain, pcm)
    assert _segs(st) == want
    rules_but_none = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    rules_but_none.set("grammar", G.GOLDEN["letters"])
    rules_but_none.c.n_grammar_rules = 0
    st.full(rules_but_none, pcm)
    assert _segs(st) == want
    count_but_null = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    count_but_null.c.n_grammar_rules = 3
    st.full(count_but_null, pcm)
    assert _segs(st) == want
    st.free()


def test_malformed_grammars_are_refused_and_the_context_goes_on(amd):
    wrs, lib = amd.wrs, amd.lib
    ctx = amd.get("s128")
    st = ctx.create_state()
    pcm = wsynth.synth_audio(480000, 0)
    logged = []
    wrs.set_log_callback(lib, lambda lvl, txt: logged.append(txt))
    try:
        for name, grammar in sorted(G.MALFORMED.items()):
            for kw in (dict(best_of=1, temperature_inc=0.0), dict(strategy=1, beam_size=5)):
                fp = wrs.FullParams(lib, kw.get("strategy", 0), **{k: v for k, v in kw.items() if k != "strategy"})
                fp.set("grammar", grammar)
                with pytest.raises(wrs.WhisperError) as ei:
                    st.full(fp, pcm)
                assert ei.value.code == ERR_GRAMMAR, (name, ei.value.code)
            assert any("grammar refused" in t for t in logged), name
            del logged[:]
    finally:
        wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    st.full(_params(wrs, lib, GOLD["cases"]["syllables_greedy"]), pcm)
    assert _segs(st) == GOLD["cases"]["syllables_greedy"]["segments"]
    st.free()


def test_full_batch_returns_the_refusal_code(amd):
    """whisper_amd_full_batch hands a malformed grammar's code back (every member refuses it before it decodes); the same states then
    transcribe in lock step under a good grammar."""
    wrs, lib, case = amd.wrs, amd.lib, GOLD["cases"]["letters_greedy"]
    ctx = amd.get("s128")
    pcms = [wsynth.synth_audio(480000, s) for s in (0, 1)]
    states = [ctx.create_state() for _ in pcms]
    bad = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    bad.set("grammar", G.MALFORMED["left_recursion_behind_empty"])
    wrs.set_log_callback(lib, None)
    try:
        with pytest.raises(wrs.WhisperError) as ei:
            wrs.full_batch(ctx, states, bad, pcms)
    finally:
        wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    assert ei.value.code == ERR_GRAMMAR
    wrs.full_batch(ctx, states, _params(wrs, lib, case), pcms)
    assert _segs(states[0]) == case["segments"]
    for st in states:
        st.free()

#!/usr/bin/env python3
"""Golden vectors for grammar-constrained decoding (whisper_full_params::grammar_rules, whisper.cpp:5479-5893): the REFERENCE ENGINE
itself (oracle/_ref/libwhisper_ref.so) on the seeded synthetic s128 / s128u models and audio seed 0, with the grammars of
tools/wgrammar.py.  Run in the build container; writes tests/golden/s128_grammar.json (data only).

Which s128u cases carry the partial-sequence path (asserted below): nonascii_beam5 and nonascii_sampled each hold a lone lead-byte token
followed by a token that starts with a continuation byte (in the sampled case the two sit in neighbouring segments of one window, with
skipped timestamp tokens between them).  nonascii_greedy does not: under the arg-max this random model repeats whole characters and ends
its window on a lone lead byte.

The audio seed is not varied (seeds 0 and 1 decode to the same ids under these grammars); the grammar and the decode mode are."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import wgrammar as G  # noqa: E402
import wsynth  # noqa: E402
import whisper_rs as W  # noqa: E402

GREEDY = dict(best_of=1, temperature_inc=0.0)
# tag -> (model shape, grammar, FullParams keywords; "strategy" 1 = beam search).  grammar_penalty 100 is the library's default.
CASES = {
    "letters_greedy":      ("s128",  "letters",   dict(GREEDY)),
    "not_greedy":          ("s128",  "not",       dict(GREEDY)),
    "syllables_greedy":    ("s128",  "syllables", dict(GREEDY)),
    "finite_greedy":       ("s128",  "finite",    dict(GREEDY)),            # the derivation completes: every stack empty, every text token rejected
    "nonascii_greedy":     ("s128u", "nonascii",  dict(GREEDY)),            # tokens that end inside a UTF-8 sequence
    "letters_ladder":      ("s128",  "letters",   dict()),                  # the defaults: best_of 5, temperature_inc 0.2
    "letters_best_of5":    ("s128",  "letters",   dict(best_of=5, temperature=0.4, temperature_inc=0.0)),
    "letters_beam5":       ("s128",  "letters",   dict(strategy=1, beam_size=5, temperature_inc=0.0)),
    "syllables_beam8":     ("s128",  "syllables", dict(strategy=1, beam_size=8)),
    "nonascii_beam5":      ("s128u", "nonascii",  dict(strategy=1, beam_size=5, temperature_inc=0.0)),
    "letters_greedy_q5_0": ("s128:q5_0", "letters", dict(GREEDY)),          # a quantised model: the same host rule behind another decode step
    "nonascii_sampled":    ("s128u", "nonascii",  dict(best_of=1, temperature=0.8, temperature_inc=0.0)),      # one decoder drawing from the distribution: varied tokens
}
LOW_TAG, LOW_SHAPE, LOW_GRAMMAR = "letters_low_penalty", "s128", "letters"


def model_file(name):
    """"s128" or "s128:q5_0" (the reference quantizer's output, wsynth.quant_model_path)."""
    return wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)


def segs(st):
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"], tids=s["tids"],
                 p=[float(x) for x in s["p"]], plog=[float(x) for x in s["plog"]]) for s in st.segments()]


def run(lib, ctx, gname, kw, penalty=None):
    kk = {k: v for k, v in kw.items() if k != "strategy"}
    fp = W.FullParams(lib, kw.get("strategy", 0), n_threads=8, **kk)
    if gname is not None:
        fp.set("grammar", G.GOLDEN[gname])
    if penalty is not None:
        fp.set("grammar_penalty", penalty)
    st = ctx.create_state()
    st.full(fp, wsynth.synth_audio(480000, 0))
    out = segs(st)
    st.free()
    return out


def held_then_broken(vocab, gname, seg, eot):
    """How many text tokens of a window's first segment obey the grammar before one breaks it: (n_obeyed, broken)."""
    acc = G.Acceptor(*G.GOLDEN[gname])
    prefix = []
    for t in seg["ids"]:
        if t >= eot:
            continue
        if t in acc.rejected_ids(vocab, eot, prefix):
            return len(prefix), True
        prefix.append(vocab[t])
    return len(prefix), False


if __name__ == "__main__":
    ref = W.load_library(os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so"))
    W.set_log_callback(ref, None)
    ctxs = {s: W.WhisperContext.new_with_params(model_file(s), W.WhisperContextParameters(ref, use_gpu=False), lib=ref) for s in ("s128", "s128u", "s128:q5_0")}
    eot = ctxs["s128"].token_eot()
    vocabs = {"s128": wsynth.synth_vocab(), "s128u": wsynth.synth_vocab("utf8")}
    gold = {"audio": dict(n_samples=480000, seed=0), "cases": {},
            "models": {s: hashlib.sha256(open(model_file(s), "rb").read()).hexdigest() for s in ctxs}}
    for tag, (shape, gname, kw) in CASES.items():
        out = run(ref, ctxs[shape], gname, kw)
        gold["cases"][tag] = dict(model=shape, grammar=gname, params=kw, penalty=100.0, segments=out)
        print(tag, len(out), sum(len(s["ids"]) for s in out), flush=True)

    # the multi-byte cases must go through the partial-sequence rules: a token that is a lone lead byte, then one that starts with a continuation
    # byte (this random model repeats itself under the arg-max, so the greedy case may have none; the beam and the sampled case must)
    v = vocabs["s128u"]
    for tag in ("nonascii_greedy", "nonascii_beam5", "nonascii_sampled"):
        flat = [t for s in gold["cases"][tag]["segments"] for t in s["ids"] if t < eot]
        pairs = [(v[a], v[b]) for a, b in zip(flat, flat[1:]) if len(v[a]) == 1 and v[a][0] >= 0xC0 and 0x80 <= v[b][0] < 0xC0]
        print(tag, "lead + continuation pairs:", len(pairs), pairs[:4])
        assert pairs or tag == "nonascii_greedy", "no lead-byte token followed by a continuation token in " + tag

    # a LOW penalty: the grammar holds for at least 3 text tokens of the first window, then a token breaks it and the grammar is off.
    # Searched here with the reference (2.0 is too low: the very first token breaks it).
    found = None
    for penalty in [3.0 + 0.5 * k for k in range(40)]:
        out = run(ref, ctxs[LOW_SHAPE], LOW_GRAMMAR, GREEDY, penalty)
        n_ok, broken = held_then_broken(vocabs[LOW_SHAPE], LOW_GRAMMAR, out[0], eot) if out else (0, False)
        print("penalty %.1f: %d text tokens obey, broken %s" % (penalty, n_ok, broken), flush=True)
        if broken and n_ok >= 3:
            found = (penalty, out)
            break
    assert found, "no penalty found at which the grammar holds for 3 tokens and then breaks"
    gold["cases"][LOW_TAG] = dict(model=LOW_SHAPE, grammar=LOW_GRAMMAR, params=GREEDY, penalty=found[0], segments=found[1])
    unconstrained = run(ref, ctxs[LOW_SHAPE], None, GREEDY)
    assert [s["ids"] for s in found[1]] != [s["ids"] for s in unconstrained]

    json.dump(gold, open(os.path.join(ROOT, "tests", "golden", "s128_grammar.json"), "w"), indent=None, separators=(",", ":"))
    print({k: (len(c["segments"]), sum(len(s["ids"]) for s in c["segments"])) for k, c in gold["cases"].items()})

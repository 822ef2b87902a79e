"""Writes tests/golden/stream_vad.json: what the REFERENCE engine (oracle/_ref/libwhisper_ref.so, on the CPU) gives for the test recording of
live sessions that cut at pauses (tests/test_stream_vad_full_gpu.py): the probabilities P of whisper_vad_detect_speech (synthetic
VAD model of tools/wsynth_vad.py), the segments S of whisper_vad_segments_from_probs for the session's whisper_vad_params, and, per utterance -
the samples [cs_to_samples(S[j].start), min(cs_to_samples(S[j].end), T)) - whisper_full's ids, text, p and plog on model s128, greedy and beam 3,
without a carried prompt and with utterance j's ids as the prompt of utterance j + 1.  Recorded results only.

The recording (13 s + 137 samples: the last window is partial, and speech is still running at the end) must show, checked here with
tools/stream_vad_ref.py: at least 4 segments, at least one made by a merge, at least one candidate removed by min_speech, none over the cap,
and the restatement's list equal to the reference's.

    python tools/gen_golden_stream_vad.py            (after __graft_entry__.build(), where the reference library is built)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import whisper_rs as W  # noqa: E402
import wsynth  # noqa: E402
import wsynth_vad as V  # noqa: E402
import stream_vad_ref as R  # noqa: E402

N_SAMPLES = 16000 * 13 + 137
BURSTS = [(0.8, 1.9), (2.05, 2.7), (4.0, 4.1), (5.0, 6.5), (8.0, 8.9), (10.2, 11.4), (12.3, 14.0)]     # seconds of "speech"; the last runs to the end
VAD = dict(threshold=0.5, min_speech_duration_ms=250, min_silence_duration_ms=100, max_speech_duration_s=30.0, speech_pad_ms=30)
CAP_MS = 30000
CONFIGS = {          # name -> strategy, whisper_full settings
    "greedy": (0, dict(best_of=1, temperature_inc=0.0, single_segment=True, no_timestamps=True, max_tokens=16, audio_ctx=256)),
    "beam3": (1, dict(beam_size=3, temperature_inc=0.0, single_segment=True, no_timestamps=True, max_tokens=16, audio_ctx=256)),
}
OUT = os.path.join(ROOT, "tests", "golden", "stream_vad.json")


def recording(seed=0):
    """tone + chirp inside BURSTS, faint noise everywhere (as wsynth_vad.synth_audio): 16 kHz mono F32"""
    rng = np.random.default_rng(3000 + seed)
    t = np.arange(N_SAMPLES, dtype=np.float64) / 16000.0
    env = np.zeros(N_SAMPLES)
    for a, b in BURSTS:
        env[(t >= a) & (t < b)] = 1.0
    x = env * (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * (500.0 + 100.0 * t) * t))
    x += 0.002 * rng.standard_normal(N_SAMPLES)
    return x.astype(np.float32)


def full_params(lib, name, prompt, **extra):
    strategy, kw = CONFIGS[name]
    kw = dict(kw, **extra)
    if prompt:
        kw["prompt_tokens"] = prompt
    return W.FullParams(lib, strategy, **kw)


def vad_params(lib):
    return W.vad_params(lib, VAD["threshold"], VAD["min_speech_duration_ms"], VAD["min_silence_duration_ms"], VAD["max_speech_duration_s"],
                        VAD["speech_pad_ms"], 0.1)


def segs(st):
    return [dict(text=s["text"].decode("latin1"), ids=s["ids"], p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]])
            for s in st.segments()]


def run_utterances(lib, ctx, name, x, S, carry, **extra):
    """whisper_full on every utterance, in order; carry: utterance j + 1 runs with every token id of utterance j's result"""
    st = ctx.create_state()
    out, prompt = [], []
    try:
        for seg in S:
            start, n = R.utterance_range(seg, len(x))
            st.full(full_params(lib, name, prompt if carry else None, **extra), x[start:start + n])
            got = segs(st)
            out.append(dict(start=start, n_samples=n, prompt=list(prompt) if carry else [], segs=got))
            prompt = [i for s in got for i in s["ids"]]
    finally:
        st.free()
    return out


def conditions(P, S):
    c = R.constants(VAD)
    raw, state = R.first_pass(P, c)
    opened = sum(1 for i, (o, b) in enumerate(state) if o and (i == 0 or not state[i - 1][0] or state[i - 1][1] != b))
    merged = []
    for s, e, _ in raw:
        if merged and s - merged[-1][1] < R.GAP:
            merged[-1][1] = e
        else:
            merged.append([s, e])
    return dict(segments=len(S), merges=len(raw) - len(merged), candidates_discarded=opened - len(raw),
                longest_ms=max([R.utterance_range(s, N_SAMPLES)[1] for s in S] + [0]) // 16, running_at_the_end=bool(state[-1][0]),
                restatement_equal=R.segments(P, VAD) == [tuple(s) for s in S] and R.capped(P, VAD, CAP_MS)[1] == 0)


def ok(c):
    return c["segments"] >= 4 and c["merges"] >= 1 and c["candidates_discarded"] >= 1 and c["longest_ms"] <= CAP_MS and c["running_at_the_end"] and c["restatement_equal"]


if __name__ == "__main__":
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")
    lib = W.load_library(ref_path)
    W.set_log_callback(lib, None)
    x = recording()
    v = W.WhisperVadContext.new(V.model_path(), lib=lib)
    P = v.detect_speech(x)
    S = [(int(a), int(b)) for a, b in v.segments_from_probs(vad_params(lib))]
    v.free()
    cond = conditions(P, S)
    print(cond, S)
    if not ok(cond):
        raise SystemExit("the recording does not meet the conditions")
    ctx = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(lib, use_gpu=False), lib=lib)
    runs = {name: {"carry%d" % c: run_utterances(lib, ctx, name, x, S, c, n_threads=8) for c in (0, 1)} for name in CONFIGS}
    ids = [i for u in runs["greedy"]["carry0"] for s in u["segs"] for i in s["ids"]]
    print("distinct ids: %d, utterances with tokens: %d" % (len(set(ids)), sum(1 for u in runs["greedy"]["carry0"] if any(s["ids"] for s in u["segs"]))))
    doc = dict(model="s128", vad_model="wsynth_vad seed 0", n_samples=N_SAMPLES, engine="reference (CPU)", vad=VAD, max_utterance_ms=CAP_MS,
               conditions="at least 4 segments, a merge, a candidate removed by min_speech, none over the cap, speech running at the end, "
                          "tools/stream_vad_ref.py equal to the reference's list",
               met=cond, P=[int(b) for b in np.asarray(P, np.float32).view(np.uint32)], S=[list(s) for s in S], configs=runs)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))

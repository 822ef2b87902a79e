"""Writes tests/golden/s128_stream.json: what the REFERENCE engine (oracle/_ref/libwhisper_ref.so, on the CPU) gives for the windows and
prompts of tools/stream_ref.py - the literal restatement of examples/stream/stream.cpp - on 12 s of wsynth audio, model s128, in the two
configurations of tests/test_stream_full_gpu.py.  The audio seed is the first one for which the reference's own run shows at least 10
distinct ids, a commit that leaves a non-empty prompt, and a window whose result differs from the previous window's.

    python tools/gen_golden_stream.py            (after __graft_entry__.build(), where the reference library is built)
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
from stream_ref import StreamRef, drive  # noqa: E402

SECONDS = 12
CONFIGS = {          # name -> (step_ms, length_ms, keep_ms), strategy, whisper_full settings
    "greedy_1000_4000_200": ((1000, 4000, 200), 0, dict(best_of=1, temperature_inc=0.0, single_segment=True, no_timestamps=True, max_tokens=16, audio_ctx=256)),
    "beam3_3000_6000_200": ((3000, 6000, 200), 1, dict(beam_size=3, temperature_inc=0.0, single_segment=True, no_timestamps=True, max_tokens=16, audio_ctx=384)),
}
OUT = os.path.join(ROOT, "tests", "golden", "s128_stream.json")


def full_params(lib, name, prompt, **extra):
    _, strategy, kw = CONFIGS[name]
    kw = dict(kw, **extra)
    if prompt:
        kw["prompt_tokens"] = prompt
    return W.FullParams(lib, strategy, **kw)


def segs(st):
    return [dict(text=s["text"].decode("latin1"), ids=s["ids"], p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]])
            for s in st.segments()]


def run_config(lib, ctx, name, audio, **extra):
    st = ctx.create_state()

    def run(pcm, prompt):
        st.full(full_params(lib, name, prompt, **extra), pcm)
        return segs(st)

    try:
        return drive(StreamRef(*CONFIGS[name][0]), audio, run)
    finally:
        st.free()


def conditions(windows):
    ids = [[i for s in w["segs"] for i in s["ids"]] for w in windows]
    return dict(distinct_ids=len({i for w in ids for i in w}),
                commits_with_prompt=sum(1 for k, w in enumerate(windows) if w["committed"] and ids[k]),
                windows_that_differ=sum(1 for a, b in zip(ids, ids[1:]) if a != b))


def ok(c):
    return c["distinct_ids"] >= 10 and c["commits_with_prompt"] >= 1 and c["windows_that_differ"] >= 1


if __name__ == "__main__":
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")
    lib = W.load_library(ref_path)
    W.set_log_callback(lib, None)
    ctx = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(lib, use_gpu=False), lib=lib)
    for seed in range(64):
        audio = wsynth.synth_audio(16000 * SECONDS, seed)
        runs = {name: run_config(lib, ctx, name, audio, n_threads=8) for name in CONFIGS}
        conds = {name: conditions(r) for name, r in runs.items()}
        print("seed %d: %r" % (seed, conds))
        if all(ok(c) for c in conds.values()):
            break
    else:
        raise SystemExit("no seed below 64 meets the conditions")
    doc = dict(model="s128", seconds=SECONDS, audio_seed=seed, engine="reference (CPU)",
               conditions="per configuration: >= 10 distinct ids, >= 1 commit with a non-empty prompt, >= 1 window that differs from the previous one",
               configs={name: dict(step_length_keep=list(CONFIGS[name][0]), met=conds[name],
                                   windows=[dict(take=w["take"], n_samples=len(w["pcm"]), prompt=w["prompt"], committed=bool(w["committed"]), segs=w["segs"])
                                            for w in runs[name]]) for name in CONFIGS})
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))

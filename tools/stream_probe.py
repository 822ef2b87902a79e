"""Measurements of the live streaming sessions (whisper_amd_stream_*) on one MI355X.

    python tools/stream_probe.py feed                       feed latency per 100 ms packet, 16 kHz F32 mono and 48 kHz I16 stereo
    python tools/stream_probe.py window --model small       from the feed that makes a window due to its results: 1 s steps, length 10 s,
                                        [--ref]             audio_ctx 512 (BASELINE config 5's cadence); --ref: the reference engine on the
                                                            host cores on the same windows and prompts, segments compared
    python tools/stream_probe.py many --model small         8 sessions per tick through step_many against the same 8 stepped one by one

--model: a wsynth shape, or shape:qtype (large-v3:q5_0).  Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import whisper_rs as W  # noqa: E402
import wsynth  # noqa: E402

STEP, LENGTH, KEEP = 1000, 10000, 200
FULL = dict(best_of=1, temperature_inc=0.0, single_segment=True, no_timestamps=True, max_tokens=32, audio_ctx=512)


def model_file(name):
    return wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)


def stats(us):
    us = sorted(us)
    return dict(n=len(us), best=round(us[0], 1), median=round(us[len(us) // 2], 1), worst=round(us[-1], 1))


def ids_of(state):
    return [s["ids"] for s in state.segments()]


def probe_feed(lib, ctx):
    for tag, kw, packet in (("16 kHz F32 mono", {}, wsynth.synth_audio(1600, 1)),
                            ("48 kHz I16 stereo", dict(sample_rate=48000, channels=2, format=W.PCM_I16),
                             np.repeat((wsynth.synth_audio(4800, 1) * 20000).astype(np.int16), 2))):
        s = W.WhisperStream(ctx, step_ms=STEP, length_ms=LENGTH, keep_ms=KEEP, **kw)
        for _ in range(20):
            s.feed(packet)
        us = []
        for _ in range(200):
            t = time.perf_counter()
            s.feed(packet)
            us.append(1e6 * (time.perf_counter() - t))
        print(json.dumps(dict(what="feed of one 100 ms packet from host memory, " + tag, unit="us", **stats(us), info=s.info())))
        s.close()


def probe_window(lib, ctx, model, seconds, with_ref):
    audio = wsynth.synth_audio(16000 * seconds, 9)
    fp = W.FullParams(lib, 0, **FULL)
    s = W.WhisperStream(ctx, step_ms=STEP, length_ms=LENGTH, keep_ms=KEEP)
    rows = []
    for k in range(seconds * 10):
        t = time.perf_counter()
        due = s.feed(audio[1600 * k:1600 * (k + 1)])
        if due > 0:
            assert s.step(fp) == 1
            ms = 1e3 * (time.perf_counter() - t)
            rows.append(dict(ms=ms, pcm=s.window(), prompt=s.prompt(), ids=ids_of(s.state)))
    s.close()
    warm = rows[2:]                                 # the first windows also pay first-use allocations
    out = dict(what="feed that makes a window due -> results, 1 s steps, length 10 s, audio_ctx 512, up to 32 tokens", model=model, unit="ms",
               windows=len(warm), tokens=sum(len(i) for r in warm for i in r["ids"]), **stats([r["ms"] for r in warm]))
    if with_ref:
        ref = W.load_library(os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so"))
        W.set_log_callback(ref, None)
        rctx = W.WhisperContext.new_with_params(model_file(model), W.WhisperContextParameters(ref, use_gpu=False), lib=ref)
        rst = rctx.create_state()
        ms, same = [], True
        for r in warm:
            kw = dict(FULL, n_threads=16)
            if r["prompt"]:
                kw["prompt_tokens"] = r["prompt"]
            t = time.perf_counter()
            rst.full(W.FullParams(ref, 0, **kw), r["pcm"])
            ms.append(1e3 * (time.perf_counter() - t))
            same = same and ids_of(rst) == r["ids"]
        out["reference_on_16_host_threads_ms"] = stats(ms)
        out["segments_identical_to_reference"] = same
        rst.free(); rctx.free()
    print(json.dumps(out))


def probe_many(lib, ctx, model, ticks):
    audios = [wsynth.synth_audio(16000 * ticks, seed) for seed in range(8)]
    fp = W.FullParams(lib, 0, **FULL)
    res = {}
    for mode in ("one by one", "step_many"):
        ss = [W.WhisperStream(ctx, step_ms=STEP, length_ms=LENGTH, keep_ms=KEEP) for _ in audios]
        ms, ids = [], []
        for k in range(ticks):
            for s, a in zip(ss, audios):
                assert s.feed(a[16000 * k:16000 * (k + 1)]) == 1
            t = time.perf_counter()
            if mode == "step_many":
                assert W.stream_step_many(ss, fp) == 8
            else:
                for s in ss:
                    assert s.step(fp) == 1
            ms.append(1e3 * (time.perf_counter() - t))
            ids.append([ids_of(s.state) for s in ss])
        res[mode] = dict(ms=ms[2:], ids=ids, batch=W.batch_stats(ctx))
        for s in ss:
            s.close()
    print(json.dumps(dict(what="8 sessions, one window each per tick (1 s steps, length 10 s, audio_ctx 512, up to 32 tokens)", model=model, unit="ms per tick",
                          one_by_one=stats(res["one by one"]["ms"]), step_many=stats(res["step_many"]["ms"]),
                          same_results=res["one by one"]["ids"] == res["step_many"]["ids"], lock_step_passes_and_rows_last_tick=res["step_many"]["batch"],
                          tokens_per_tick=sum(len(i) for sess in res["step_many"]["ids"][-1] for i in sess))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["feed", "window", "many"])
    ap.add_argument("--model", default="small")
    ap.add_argument("--seconds", type=int, default=14)
    ap.add_argument("--ref", action="store_true")
    args = ap.parse_args()
    lib = W.load_library()
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    ctx = W.WhisperContext.new_with_params(model_file(args.model), W.WhisperContextParameters(lib, flash_attn=False), lib=lib)
    if args.what == "feed":
        probe_feed(lib, ctx)
    elif args.what == "window":
        probe_window(lib, ctx, args.model, args.seconds, args.ref)
    else:
        probe_many(lib, ctx, args.model, args.seconds)
    ctx.free()

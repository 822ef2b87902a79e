#!/usr/bin/env python3
"""Times the three ways to transcribe a long recording with VAD, in one session on one context: whisper_full(vad = true),
whisper_full_parallel(vad = true, 8) and whisper_amd_full_long(..., 30 s, 8).  The recording is the synthetic VAD test audio (14 s, five
bursts) repeated to N minutes; the models are synthetic (tools/wsynth.py, tools/wsynth_vad.py).  Prints one JSON line: the best wall time
of each call, the audio-seconds-per-second it amounts to, the segment counts, and for whisper_amd_full_long the split of
whisper_amd_long_stats (VAD, plan + pack, transcription, waves, chunks, PCM bytes uploaded) with the VAD's share of the call.

  python tools/long_probe.py [--minutes 20] [--model s128] [--reps 2] [--n-parallel 8] [--max-chunk-ms 30000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import wsynth  # noqa: E402
import wsynth_vad as V  # noqa: E402
import whisper_rs as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=20.0)
    ap.add_argument("--model", default="s128")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--n-parallel", type=int, default=8)
    ap.add_argument("--max-chunk-ms", type=int, default=30000)
    a = ap.parse_args()

    lib = W.load_library()
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 4 else None)
    short = V.synth_audio()
    n = int(a.minutes * 60 * 16000)
    pcm = np.ascontiguousarray(np.tile(short, -(-n // len(short)))[:n])
    seconds = len(pcm) / 16000.0
    ctx = W.WhisperFullContext.new_with_params(wsynth.model_path(a.model), W.WhisperContextParameters(lib, flash_attn=False), lib=lib)

    def fp(vad):
        return W.FullParams(lib, best_of=1, temperature_inc=0.0, vad=vad, vad_model_path=V.model_path())

    calls = {
        "whisper_full_vad": lambda x: ctx.full(fp(True), x),
        "whisper_full_parallel_vad_8": lambda x: ctx.full_parallel(fp(True), x, 8),
        "whisper_amd_full_long": lambda x: ctx.full_long(fp(False), x, a.max_chunk_ms, a.n_parallel),
    }
    res = dict(minutes=a.minutes, model=a.model, audio_s=seconds)
    for name, call in calls.items():
        assert call(short) == 0                              # first use: code objects, the VAD context, the batcher
        runs, extra = [], {}
        for _ in range(a.reps):
            w0 = time.perf_counter()
            rc = call(pcm)
            wall = time.perf_counter() - w0
            assert rc == 0, (name, rc)
            if not runs or wall < min(runs):
                extra = dict(segments=lib.whisper_full_n_segments(ctx.ptr), tokens=sum(lib.whisper_full_n_tokens(ctx.ptr, i)
                                                                                       for i in range(lib.whisper_full_n_segments(ctx.ptr))))
                if name == "whisper_amd_full_long":
                    s = ctx.long_stats()
                    extra.update(stats=s, lockstep=ctx.batch_stats(), vad_share=round(s["vad_us"] / (wall * 1e6), 4),
                                 chunk_samples=[c["packed"] for c in ctx.long_chunks()][:4])
            runs.append(wall)
        res[name] = dict(best_s=round(min(runs), 4), runs_s=[round(r, 4) for r in runs], x_real_time=round(seconds / min(runs), 1), **extra)
    # what whisper_amd_full_long spends on the member states it makes and releases per call (inside its transcription time)
    w0 = time.perf_counter()
    extra_states = [lib.whisper_init_state(ctx.ptr) for _ in range(a.n_parallel - 1)]
    for s in extra_states:
        lib.whisper_free_state(s)
    res["member_states_make_release_ms"] = round((time.perf_counter() - w0) * 1e3, 3)
    ctx.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

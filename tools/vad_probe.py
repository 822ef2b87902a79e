#!/usr/bin/env python3
"""Times whisper_vad_detect_speech of the product and of the reference engine (oracle/_ref/libwhisper_ref.so, 4 threads: its default
for VAD) on the synthetic VAD model: the 14 s test audio (438 windows) and 30 minutes of it repeated (56 250 windows).  Prints one JSON
line; the product's split between waiting for the device and the host recurrence comes from whisper_amd_vad_timings.

  python tools/vad_probe.py [--no-ref] [--reps 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import wsynth_vad as V  # noqa: E402
import whisper_rs as W  # noqa: E402


def timings(lib, v):
    out = (C.c_int64 * 3)()
    lib.whisper_amd_vad_timings.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.whisper_amd_vad_timings.restype = None
    lib.whisper_amd_vad_timings(v.ptr, out)
    return [int(x) for x in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    mp, pcm = V.model_path(), V.synth_audio()
    long_pcm = np.tile(pcm, -(-30 * 60 * 16000 // len(pcm)))[:30 * 60 * 16000]
    inputs = {"438_windows": pcm, "30_min": long_pcm}
    res = {}

    lib = W.load_library()
    W.set_log_callback(lib, None)
    v = W.WhisperVadContext.new(mp, lib=lib)
    v.detect_speech(pcm)                                     # first launch: code object load
    for tag, x in inputs.items():
        runs = []
        for _ in range(a.reps):
            t0 = timings(lib, v)
            w0 = time.perf_counter()
            p = v.detect_speech(x)
            wall = time.perf_counter() - w0
            t1 = timings(lib, v)
            runs.append(dict(wall_ms=wall * 1e3, device_wait_ms=(t1[1] - t0[1]) / 1e3, host_recurrence_ms=(t1[2] - t0[2]) / 1e3))
        best = min(runs, key=lambda r: r["wall_ms"])
        res[tag] = dict(windows=len(p), product=best, product_runs_ms=[round(r["wall_ms"], 3) for r in runs])
        # the front end alone, all slabs, results copied to the host
        w0 = time.perf_counter()
        v.front(x)
        res[tag]["product_front_only_ms"] = (time.perf_counter() - w0) * 1e3
        res[tag]["bits_head"] = [int(b) for b in p[:4].view(np.uint32)]
    v.free()

    ref_path = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")
    if not a.no_ref and os.path.exists(ref_path):
        ref = W.load_library(ref_path)
        W.set_log_callback(ref, None)
        r = W.WhisperVadContext.new(mp, lib=ref, n_threads=4)
        r.detect_speech(pcm)
        for tag, x in inputs.items():
            runs = []
            for _ in range(a.reps if tag == "438_windows" else 1):
                w0 = time.perf_counter()
                p = r.detect_speech(x)
                runs.append((time.perf_counter() - w0) * 1e3)
            res[tag]["reference_4_threads_ms"] = min(runs)
            res[tag]["same_head"] = [int(b) for b in p[:4].view(np.uint32)] == res[tag]["bits_head"]
        r.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

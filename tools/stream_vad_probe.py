"""Measurements of live sessions that cut at pauses (whisper_amd_stream_open_vad) on one MI355X.

    python tools/stream_vad_probe.py front                  the front end of one poll, 100 ms of new audio (3 windows) per session, 1 and 8
                                                            sessions: ONE k_stream_vad_front launch against the pieces that existed before
                                                            (per session a k_stream_window gather into staging, a k_vad_front launch, a copy of
                                                            its result to the host), through tests/native/libstream_vad_kernels.so
    python tools/stream_vad_probe.py latency --model small  from the feed that completes an utterance to its result, 100 ms packets
    python tools/stream_vad_probe.py share                  a 60 s recording: the share of its audio that is decoded at all, against step mode's
                                                            length_ms / step_ms on the same recording

The VAD model is the synthetic one of tools/wsynth_vad.py, the recording tools/gen_golden_stream_vad.py's bursts.  Prints one JSON line per
measurement.
"""
import argparse
import ctypes as C
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
import wsynth_vad as V  # noqa: E402
import gen_golden_stream_vad as GG  # noqa: E402

FULL = dict(best_of=1, temperature_inc=0.0, single_segment=True, no_timestamps=True, max_tokens=32, audio_ctx=256)
STEP_MODE = (3000, 10000)            # whisper_amd_stream_default_params: step_ms, length_ms


def stats(us):
    us = sorted(us)
    return dict(n=len(us), best=round(us[0], 1), median=round(us[len(us) // 2], 1), worst=round(us[-1], 1))


def probe_front(iters=200):
    h = C.CDLL(os.path.join(ROOT, "tests", "native", "libstream_vad_kernels.so"))
    t = dict(V.tensors())
    u16 = lambda name: np.ascontiguousarray(t[name]).view(np.uint16).reshape(-1)
    f32 = lambda name: np.ascontiguousarray(t[name], np.float32).reshape(-1)
    arrs = [u16("_model.stft.forward_basis_buffer")] + [u16("_model.encoder.%d.reparam_conv.weight" % i) for i in range(4)] + \
           [f32("_model.encoder.%d.reparam_conv.bias" % i) for i in range(4)] + [f32("_model.decoder.rnn.weight_ih"), f32("_model.decoder.rnn.bias_ih")]
    h.svtest_set_weights.argtypes = [C.c_void_p] * 11
    assert h.svtest_set_weights(*[a.ctypes.data for a in arrs]) == 0
    h.svtest_time.argtypes = [C.c_int] * 5 + [C.c_void_p]
    for n in (1, 8):
        res = {}
        for rep in range(3):                             # the two forms alternate: a drifting clock or a busy neighbour hits both
            for mode, tag in ((0, "one_launch"), (1, "gather_front_copy_per_session")):
                us = np.zeros(iters, np.float64)
                assert h.svtest_time(mode, n, 3, 480000 + 640000, iters, us.ctypes.data) == 0
                res.setdefault(tag, []).extend(us.tolist())
        a, b = stats(res["one_launch"]), stats(res["gather_front_copy_per_session"])
        print(json.dumps(dict(what="front end of one poll: %d session(s) x 3 new windows, launch to gate inputs on the host" % n, unit="us", one_launch=a,
                              gather_front_copy_per_session=b, ratio_of_medians=round(b["median"] / a["median"], 2))))


def long_recording(seconds=60):
    reps = -(-seconds * 16000 // GG.N_SAMPLES)
    return np.concatenate([GG.recording(seed) for seed in range(reps)])[:seconds * 16000]


def probe_latency(lib, ctx, vctx, model):
    a = long_recording(39)
    fp = W.FullParams(lib, 0, **FULL)
    s = W.WhisperVadStream(ctx, vctx)
    ms, feed_us, n_samples = [], [], []
    for k in range(len(a) // 1600):
        t = time.perf_counter()
        due = s.feed(a[1600 * k:1600 * (k + 1)])
        feed_us.append(1e6 * (time.perf_counter() - t))
        while due > 0:
            assert s.step(fp) == 1
            ms.append(1e3 * (time.perf_counter() - t))
            n_samples.append(s.utterance_info()["length"])
            due = s.pending()
    s.close()
    print(json.dumps(dict(what="feed that completes an utterance -> its result (100 ms packets, audio_ctx 256, up to 32 tokens)", model=model, unit="ms",
                          utterances=len(ms), utterance_ms=[n // 16 for n in n_samples], **stats(ms[1:]),
                          feed_with_vad_us=stats(feed_us[20:]))))


def probe_share(lib, ctx, vctx):
    a = long_recording(60)
    s = W.WhisperVadStream(ctx, vctx)
    fp = W.FullParams(lib, 0, **FULL)
    decoded = 0
    for k in range(len(a) // 1600):
        s.feed(a[1600 * k:1600 * (k + 1)])
        while s.pending() > 0:
            assert s.step(fp) == 1
            decoded += s.utterance_info()["length"]
    s.flush()
    while s.pending() > 0:
        assert s.step(fp) == 1
        decoded += s.utterance_info()["length"]
    n_utt = s.utterance_info()["utterances"]
    s.close()
    step, length = STEP_MODE
    windows = len(a) // (16 * step)
    step_decoded = sum(min(length, (k + 1) * step) for k in range(windows)) * 16
    print(json.dumps(dict(what="60 s recording: samples handed to whisper_full / samples fed", utterances=n_utt, vad_mode=round(decoded / len(a), 3),
                          step_mode=round(step_decoded / len(a), 3), step_mode_settings=dict(step_ms=step, length_ms=length),
                          step_mode_steady_state=round(length / step, 3))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["front", "latency", "share"])
    ap.add_argument("--model", default="small")
    args = ap.parse_args()
    if args.what == "front":
        probe_front()
        sys.exit(0)
    lib = W.load_library()
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    ctx = W.WhisperContext.new_with_params(wsynth.model_path(args.model), W.WhisperContextParameters(lib, flash_attn=False), lib=lib)
    vctx = W.WhisperVadContext.new(V.model_path(), lib=lib)
    if args.what == "latency":
        probe_latency(lib, ctx, vctx, args.model)
    else:
        probe_share(lib, ctx, vctx)
    vctx.free()
    ctx.free()

#!/usr/bin/env python3
"""Times the two-channel calls on one device, in one session.  Prints one JSON line with three sets of timings:

  split   device time of ONE whisper_amd_audio_split launch, between two HIP events on the state's stream (device-pointer input, so that nothing
          but the kernel lies between the events), against the two whisper_amd_audio_to_pcm calls a caller makes today on the channels it
          extracted on the host (two launches between the same kind of events): 16 kHz F32, 8 kHz int16 and 44.1 kHz int16, --seconds each.
  full    wall time of whisper_amd_full_long_channels against what a caller does without it: de-interleave on the host, two
          whisper_amd_audio_to_pcm calls, two whisper_amd_full_long calls; the stereo recording is tools/channels_cases.two_speakers repeated
          --repeat times at a cap of --max-chunk-ms (3 chunks per channel and repeat); waves on both sides.
  stages  the share of the channels call spent in the two VAD passes (whisper_amd_long_stats), in plan + pack, in transcription.

  python tools/channels_probe.py [--seconds 60] [--repeat 1] [--max-chunk-ms 3000] [--model s128] [--reps 5]
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
import channels_cases as K  # noqa: E402
import wsynth  # noqa: E402
import wsynth_vad as V  # noqa: E402
import whisper_rs as W  # noqa: E402


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")

    def ok(self, rc):
        assert rc == 0, "HIP error %d" % rc

    def device_copy(self, x):
        p = C.c_void_p()
        self.ok(self.lib.hipMalloc(C.byref(p), C.c_size_t(x.nbytes + 256)))
        self.ok(self.lib.hipMemcpy(p, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1))
        return p

    def timed(self, stream, fn, reps):
        """best device time in microseconds of fn()'s work on `stream`, between two events"""
        e0, e1, best = C.c_void_p(), C.c_void_p(), None
        self.ok(self.lib.hipEventCreate(C.byref(e0))); self.ok(self.lib.hipEventCreate(C.byref(e1)))
        for k in range(reps + 1):                           # the first run loads code objects and tables: not counted
            self.ok(self.lib.hipEventRecord(e0, C.c_void_p(stream)))
            fn()
            self.ok(self.lib.hipEventRecord(e1, C.c_void_p(stream)))
            self.ok(self.lib.hipEventSynchronize(e1))
            ms = C.c_float(0.0)
            self.ok(self.lib.hipEventElapsedTime(C.byref(ms), e0, e1))
            if k > 0:
                best = ms.value if best is None else min(best, ms.value)
        self.lib.hipEventDestroy(e0); self.lib.hipEventDestroy(e1)
        return round(best * 1e3, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--max-chunk-ms", type=int, default=3000)
    ap.add_argument("--model", default="s128")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()

    lib = W.load_library()
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 4 else None)
    hip = Hip()
    ctx = W.WhisperFullContext.new_with_params(wsynth.model_path(a.model), W.WhisperContextParameters(lib, flash_attn=False), lib=lib)
    st = W.WhisperState(ctx, ctx.state_ptr())
    lib.whisper_amd_state_stream.restype = C.c_void_p           # a pointer: ctypes' default int result would cut the handle to 32 bits
    lib.whisper_amd_state_stream.argtypes = [C.c_void_p]
    stream = lib.whisper_amd_state_stream(st.ptr)
    assert stream
    res = dict(model=a.model, seconds=a.seconds)

    # (a) the split
    rng = np.random.default_rng(1)
    res["split"] = {}
    for tag, rate, fmt in (("f32_16k", 16000, W.PCM_F32), ("i16_8k", 8000, W.PCM_I16), ("i16_44k1", 44100, W.PCM_I16)):
        nf = int(a.seconds * rate)
        x = rng.uniform(-0.5, 0.5, 2 * nf).astype(np.float32)
        if fmt == W.PCM_I16:
            x = K.to_i16(x)
        d = hip.device_copy(x)
        d0, d1 = hip.device_copy(K.channel(x, 0)), hip.device_copy(K.channel(x, 1))
        one = hip.timed(stream, lambda: st.audio_split((d.value, nf), rate, fmt), a.reps)

        def two():
            st.audio_to_pcm((d0.value, nf), 1, rate, fmt)
            st.audio_to_pcm((d1.value, nf), 1, rate, fmt)
        res["split"][tag] = dict(split_us=one, two_mono_calls_us=hip.timed(stream, two, a.reps))
        for p in (d, d0, d1):
            hip.lib.hipFree(p)

    # (b) the whole call, (c) its stages
    x = np.tile(K.two_speakers().reshape(-1, 2), (a.repeat, 1)).reshape(-1)
    fp = W.FullParams(lib, best_of=1, temperature_inc=0.0, vad_model_path=V.model_path())

    def channels():
        assert ctx.full_long_channels(fp, x, 16000, None, a.max_chunk_ms, 8) == 0
        return ctx.channels_stats()["waves"], lib.whisper_full_n_segments(ctx.ptr)

    def by_hand():
        waves = segs = 0
        for c in (0, 1):
            ptr, n = st.audio_to_pcm(K.channel(x, c), 1, 16000)         # the host de-interleave is part of what the caller does
            assert ctx.full_long(fp, (ptr, n), a.max_chunk_ms, 8) == 0
            waves += ctx.long_stats()["waves"]
            segs += lib.whisper_full_n_segments(ctx.ptr)
        return waves, segs

    full = {}
    for name, call in (("channels", channels), ("two_full_long", by_hand)):
        call()                                                           # first use: the VAD context, the batcher, member states' code
        best, info, stages = None, None, None
        for _ in range(a.reps):
            w0 = time.perf_counter()
            info = call()
            wall = time.perf_counter() - w0
            if best is None or wall < best:
                best = wall
                if name == "channels":
                    s = ctx.long_stats()
                    stages = dict(vad_us=s["vad_us"], pack_us=s["pack_us"], transcribe_us=s["transcribe_us"],
                                  vad_share=round(s["vad_us"] / (wall * 1e6), 4), stats=ctx.channels_stats())
        full[name] = dict(best_ms=round(best * 1e3, 2), waves=info[0], segments=info[1])
        if stages:
            res["stages"] = stages
    full["audio_s_per_channel"] = len(x) / 2 / 16000.0
    res["full"] = full
    ctx.free()
    print(json.dumps(res))


if __name__ == "__main__":
    main()

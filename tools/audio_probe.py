"""Time of the audio front end for 30 s of 48 kHz stereo int16, the device path beside the host restatement, in ONE process.

  to_pcm     whisper_amd_audio_to_pcm on a recording that lies in device memory: DEVICE time between two HIP events on the state's stream
             (the resampling kernel alone), and the same call's wall time with the recording in host memory (upload + kernel + wait).
  host       the same call on a state created with WHISPER_AMD_AUDIO_HOST=1: wa_audio_ref on the host, then the upload.  Wall time.
  full       whisper_amd_full_audio (small shape, greedy, temperature_inc 0) on the device state, beside audio_to_pcm on the host state
             followed by full() on a host copy of its result - what a caller without the front end does.  Wall time.

`--calls` calls each after one warm-up call, alternating, best and median, printed as one JSON line.

`--format i16,f32,u8,s24,s32,f64,ulaw,alaw` (any of them) measures the sample formats instead: the same recording (`--seconds`, `--channels`, `--rate`)
rendered in each format, lying in device memory, through whisper_amd_audio_to_pcm - DEVICE time between two HIP events, the formats taken in
turn within every round after one warm-up round - with the bytes a caller uploads for it, as one JSON line.
usage: python tools/audio_probe.py [--calls 10] [--shape small] [--rate 48000] [--format LIST [--seconds 60] [--channels 1]]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import numpy as np  # noqa: E402
import wsynth, whisper_rs as W  # noqa: E402


def summary(ms):
    return {"best_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "calls": len(ms)}


def recording(rate, seconds=30):
    """a fixed stereo int16 rendering of the synthetic audio at `rate`"""
    pcm = wsynth.synth_audio(16000 * seconds, 0)
    n = rate * seconds
    up = np.interp(np.arange(n) * (16000.0 / rate), np.arange(len(pcm)), pcm)
    scale = 0.8 * 32767.0 / float(np.abs(up).max())
    return np.stack([np.rint(up * scale), np.rint(up * scale * 0.7)], axis=1).astype(np.int16).reshape(-1)


FORMATS = {"i16": W.PCM_I16, "f32": W.PCM_F32, "u8": W.PCM_U8, "s24": W.PCM_S24, "s32": W.PCM_S32, "f64": W.PCM_F64, "ulaw": W.PCM_ULAW, "alaw": W.PCM_ALAW}


def rendered(x, name):
    """the int16 samples `x` in format `name`, as the array the entry reads"""
    s = x.astype(np.int32)
    return {"i16": lambda: x, "f32": lambda: (s / 32768.0).astype(np.float32), "u8": lambda: ((s >> 8) + 128).astype(np.uint8), "s24": lambda: W.pack_s24(s << 8),
            "s32": lambda: (s << 16).astype(np.int32), "f64": lambda: s / 32768.0, "ulaw": lambda: W.linear_to_ulaw(x), "alaw": lambda: W.linear_to_alaw(x)}[name]()


def probe_formats(a):
    names = a.format.split(",")
    assert all(n in FORMATS for n in names), "--format takes a list of %s" % ", ".join(FORMATS)
    lib = W.load_library()
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    hip = C.CDLL("libamdhip64.so")
    lib.whisper_amd_state_stream.restype = C.c_void_p
    lib.whisper_amd_state_stream.argtypes = [C.c_void_p]
    ctx = W.WhisperContext.new_with_params(wsynth.model_path(a.shape), W.WhisperContextParameters(lib, gpu_device=0), lib=lib)
    st = ctx.create_state()
    x = recording(a.rate, a.seconds)
    if a.channels == 1:
        x = np.ascontiguousarray(x[0::2])
    n_frames = len(x) // a.channels
    bufs = {}
    for n in names:
        r = np.ascontiguousarray(rendered(x, n)).reshape(-1)
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(r.nbytes)) == 0 and hip.hipMemcpy(d, C.c_void_p(r.ctypes.data), C.c_size_t(r.nbytes), 1) == 0
        bufs[n] = (d, r.nbytes)
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    stream = C.c_void_p(lib.whisper_amd_state_stream(st.ptr))
    t = {n: [] for n in names}
    for it in range(a.calls + 1):
        for n in names:
            assert hip.hipEventRecord(e0, stream) == 0
            st.audio_to_pcm((bufs[n][0].value, n_frames), a.channels, a.rate, FORMATS[n])
            assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
            if it > 0:
                t[n].append(ms.value)
    out = {"rate": a.rate, "channels": a.channels, "seconds": a.seconds, "n_frames": n_frames, "n_samples": int(lib.whisper_amd_audio_n_samples(n_frames, a.rate)),
           "stats": st.audio_stats(),
           "formats": {n: dict(summary(t[n]), worst_ms=round(max(t[n]), 3), upload_bytes=bufs[n][1]) for n in names}}
    for d, _ in bufs.values():
        hip.hipFree(d)
    st.free(); ctx.free()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--shape", default="small")
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--format", default=None)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--channels", type=int, default=1, choices=(1, 2))
    a = ap.parse_args()
    if a.format:
        return probe_formats(a)
    lib = W.load_library()
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    hip = C.CDLL("libamdhip64.so")
    lib.whisper_amd_state_stream.restype = C.c_void_p
    lib.whisper_amd_state_stream.argtypes = [C.c_void_p]
    ctx = W.WhisperContext.new_with_params(wsynth.model_path(a.shape), W.WhisperContextParameters(lib, gpu_device=0), lib=lib)
    dev = ctx.create_state()
    os.environ["WHISPER_AMD_AUDIO_HOST"] = "1"          # the switch is read when a state is created
    host = ctx.create_state()
    os.environ.pop("WHISPER_AMD_AUDIO_HOST")
    x = recording(a.rate)
    n_frames = len(x) // 2
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(x.nbytes)) == 0
    assert hip.hipMemcpy(d, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0
    e0, e1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(e0)) == 0 and hip.hipEventCreate(C.byref(e1)) == 0
    stream = C.c_void_p(lib.whisper_amd_state_stream(dev.ptr))
    fp = W.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    t = {k: [] for k in ("to_pcm_device_time", "to_pcm_wall_host_input", "host_restatement_wall", "full_audio_wall", "host_restatement_then_full_wall")}
    segs = {}
    for it in range(a.calls + 1):
        assert hip.hipEventRecord(e0, stream) == 0
        dev.audio_to_pcm((d.value, n_frames), 2, a.rate, W.PCM_I16)
        assert hip.hipEventRecord(e1, stream) == 0 and hip.hipEventSynchronize(e1) == 0
        ms = C.c_float()
        assert hip.hipEventElapsedTime(C.byref(ms), e0, e1) == 0
        w0 = time.perf_counter(); dev.audio_to_pcm(x, 2, a.rate); w1 = time.perf_counter()
        host.audio_to_pcm(x, 2, a.rate); w2 = time.perf_counter()
        dev.full_audio(fp, x, 2, a.rate); w3 = time.perf_counter()
        segs["device"] = [(s["t0"], s["t1"], s["ids"]) for s in dev.segments()]
        w4 = time.perf_counter()
        host.audio_to_pcm(x, 2, a.rate)
        host.full(fp, host.audio_copy()); w5 = time.perf_counter()
        segs["host"] = [(s["t0"], s["t1"], s["ids"]) for s in host.segments()]
        if it > 0:
            for k, v in zip(t, (ms.value, (w1 - w0) * 1e3, (w2 - w1) * 1e3, (w3 - w2) * 1e3, (w5 - w4) * 1e3)):
                t[k].append(v)
    out = {k: summary(v) for k, v in t.items()}
    out.update(rate=a.rate, shape=a.shape, n_frames=n_frames, n_samples=int(lib.whisper_amd_audio_n_samples(n_frames, a.rate)),
               same_result=segs["device"] == segs["host"], stats_device_state=dev.audio_stats(), stats_host_state=host.audio_stats())
    hip.hipFree(d)
    dev.free(); host.free(); ctx.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

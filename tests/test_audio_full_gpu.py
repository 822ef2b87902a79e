"""whisper_amd_full_audio and the stream-ordered hand-off of whisper_amd_audio_to_pcm's buffer, on the s128 model and the 30 s synthetic audio.

At 16 kHz the front end is the whisper-rs utilities (numpy restatements in whisper_rs.py), so transcribing an int16 stereo recording through it
gives what full() gives on the converted audio, field for field and with the same mel; for mono F32 that is the reference engine's golden.  At
48 kHz it gives what full() gives on wa_audio_ref's output of the same recording (the restatement that tests/test_audio_kernels_gpu.py holds
the kernels to and tests/test_audio_math.py holds to float64)."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import wsynth
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(ROOT, "tests", "native", "libaudio_kernels.so")
I16, F32 = 0, 1


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def get_mel(lib, st):
    lib.whisper_amd_get_mel.restype = C.c_int64
    lib.whisper_amd_get_mel.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    nl, nm = C.c_int(), C.c_int()
    n = lib.whisper_amd_get_mel(st.ptr, None, 0, nl, nm)
    out = np.empty(n, np.float32)
    lib.whisper_amd_get_mel(st.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n, nl, nm)
    return out, nl.value, nm.value


def fields(st):
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"], ids=s["ids"], tids=s["tids"], p=[np.float32(x).tobytes() for x in s["p"]],
                 plog=[np.float32(x).tobytes() for x in s["plog"]], no_speech=np.float32(s["no_speech_prob"]).tobytes()) for s in st.segments()]


def audio_ref(x, n_frames, ch, rate, fmt):
    lib = C.CDLL(HARNESS)
    lib.atest_ref.restype = C.c_longlong
    lib.atest_ref.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p]
    n = -(-n_frames * 16000 // rate)
    out = np.full(n, np.nan, np.float32)
    assert lib.atest_ref(x.ctypes.data, n_frames, ch, rate, fmt, out.ctypes.data) == n
    return out


@pytest.fixture(scope="module")
def env(wrs, amd_lib):
    gold = json.load(open(os.path.join(GOLDEN, "s128.json")))
    mp = wsynth.model_path("s128", gold["model_seed"])
    assert hashlib.sha256(open(mp, "rb").read()).hexdigest() == gold["model_sha256"]
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    pcm = wsynth.synth_audio(480000, 0)
    yield dict(wrs=wrs, lib=amd_lib, ctx=ctx, gold=gold, pcm=pcm)
    ctx.free()


def params(env):
    return env["wrs"].FullParams(env["lib"], 0, best_of=1, temperature_inc=0.0)


def stereo_i16(pcm, seed):
    """a fixed int16 stereo recording of a mono F32 signal: the two channels carry it at different levels, each with its own seeded noise"""
    rng = np.random.default_rng(seed)
    scale = 0.8 * 32767.0 / max(1e-9, float(np.abs(pcm).max()))
    l = np.clip(np.rint(pcm * scale + rng.normal(0.0, 2.0, len(pcm))), -32768, 32767)
    r = np.clip(np.rint(pcm * scale * 0.7 + rng.normal(0.0, 2.0, len(pcm))), -32768, 32767)
    return np.stack([l, r], axis=1).astype(np.int16).reshape(-1)


def test_16k_i16_stereo_is_full_on_the_converted_audio(env):
    wrs, lib, ctx = env["wrs"], env["lib"], env["ctx"]
    x = stereo_i16(env["pcm"], 21)
    mono = wrs.convert_stereo_i16_to_mono_f32(x)
    a, b = ctx.create_state(), ctx.create_state()
    a.full_audio(params(env), x, 2, 16000)
    b.full(params(env), mono)
    assert a.audio_copy().tobytes() == mono.tobytes()
    fa, fb = fields(a), fields(b)
    assert len(fa) > 0 and fa == fb
    mel_a, mel_b = get_mel(lib, a), get_mel(lib, b)
    assert mel_a[1:] == mel_b[1:] and digest(mel_a[0]) == digest(mel_b[0])
    assert a.audio_stats() == (1, 0, 0)
    a.free(); b.free()


def test_16k_f32_mono_is_the_golden(env):
    ctx, gold = env["ctx"], env["gold"]
    st = ctx.create_state()
    st.full_audio(params(env), env["pcm"], 1, 16000)
    want = gold["full"]["greedy_tinc0_seed0"]
    got = st.segments()
    assert len(got) == len(want) > 0
    for g, w in zip(got, want):
        assert (g["t0"], g["t1"], g["ids"], g["text"].decode("latin1")) == (w["t0"], w["t1"], w["ids"], w["text"])
        assert g["tids"] == w["tids"] and [float(np.float32(v)) for v in g["p"]] == w["p"] and [float(np.float32(v)) for v in g["plog"]] == w["plog"]
    st.free()


def test_48k_i16_stereo_is_full_on_the_restatement(env):
    wrs, lib, ctx = env["wrs"], env["lib"], env["ctx"]
    pcm = env["pcm"]
    up = np.interp(np.arange(3 * len(pcm)) / 3.0, np.arange(len(pcm)), pcm).astype(np.float32)        # a fixed 48 kHz rendering of the signal
    x = stereo_i16(up, 22)
    n_frames = len(x) // 2
    want_pcm = audio_ref(x, n_frames, 2, 48000, I16)
    assert len(want_pcm) == 480000 and np.all(np.isfinite(want_pcm))
    a, b = ctx.create_state(), ctx.create_state()
    a.full_audio(params(env), x, 2, 48000)
    assert a.audio_copy().tobytes() == want_pcm.tobytes()
    b.full(params(env), want_pcm)
    fa, fb = fields(a), fields(b)
    assert len(fa) > 0 and fa == fb
    assert digest(get_mel(lib, a)[0]) == digest(get_mel(lib, b)[0])
    assert a.audio_stats() == (1, 0, 0)
    # a recording in device memory goes the same way (on a state of its own: every call here is a state's first)
    hip = C.CDLL("libamdhip64.so")
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(x.nbytes)) == 0
    assert hip.hipMemcpy(d, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0
    c = ctx.create_state()
    c.full_audio(params(env), (d.value, n_frames), 2, 48000, I16)
    assert fields(c) == fb and c.audio_stats() == (1, 0, 0)
    hip.hipFree(d)
    a.free(); b.free(); c.free()


def test_to_pcm_then_mel_without_synchronisation(env):
    """device input: nothing waits between the front end's kernel and the mel kernel but the state's stream"""
    wrs, lib, ctx = env["wrs"], env["lib"], env["ctx"]
    x = stereo_i16(env["pcm"][:160000], 23)
    mono = wrs.convert_stereo_i16_to_mono_f32(x)
    hip = C.CDLL("libamdhip64.so")
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(x.nbytes)) == 0
    assert hip.hipMemcpy(d, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0
    a, b = ctx.create_state(), ctx.create_state()
    for rate, want in ((16000, mono), (44100, audio_ref(x, len(x) // 2, 2, 44100, I16))):
        ptr, n = a.audio_to_pcm((d.value, len(x) // 2), 2, rate, I16)
        a.pcm_to_mel_device(ptr, n)
        b.pcm_to_mel(want)
        mel_a, mel_b = get_mel(lib, a), get_mel(lib, b)
        assert n == len(want) and mel_a[1:] == mel_b[1:] and digest(mel_a[0]) == digest(mel_b[0])
    hip.hipFree(d)
    a.free(); b.free()

"""Voice activity detection on the MI355X, through the C ABI: whisper_vad_* and whisper_full(vad = true) against what the reference
engine produced for the same seeded inputs (tests/golden/vad.json, tools/gen_golden_vad.py; the live reference library as well where
it is built).  Everything is compared bit for bit: the kernel's gate inputs by SHA-256 against the scalar restatement of
tests/native/vad_math.cpp (which tests/test_vad_math.py pins to the reference), probabilities as u32 patterns, segments, mapped
segment times and token ids as integers."""
import ctypes as C
import hashlib
import json
import os
import threading

import numpy as np
import pytest

import wsynth
import wsynth_vad as V
from conftest import GOLDEN, REF_LIB

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLDEN, "vad.json")))
SR = 16000


def bits(a):
    return [int(x) for x in np.asarray(a, dtype=np.float32).view(np.uint32)]


def segs_int(s):
    return [[int(a), int(b)] for a, b in s]


@pytest.fixture(scope="module")
def inputs():
    mp, pcm = V.model_path(), V.synth_audio()
    assert hashlib.sha256(open(mp, "rb").read()).hexdigest() == G["model_sha256"], "the synthetic VAD model is not the recorded one"
    assert hashlib.sha256(pcm.tobytes()).hexdigest() == G["audio_sha256"], "the synthetic audio is not the recorded one"
    return mp, pcm


@pytest.fixture(scope="module")
def vad(wrs, amd_lib, inputs):
    v = wrs.WhisperVadContext.new(inputs[0], lib=amd_lib)
    yield v
    v.free()


def check_front(got, g):
    assert got.shape == (g["n_chunks"], 512)
    for r, want in g["rows"].items():
        assert bits(got[int(r), ::64]) == want, "window %s differs" % r
    assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == g["sha256"]


# ---- the front end alone ----
def test_tile_constant(amd_lib):
    assert amd_lib.whisper_amd_vad_tile() == G["tile"], "regenerate tests/golden/vad.json for the new tile (tools/gen_golden_vad.py: TILE)"


@pytest.mark.parametrize("rel", [None, -1, 0, 1, "full"])
def test_front_end_digest(amd_lib, vad, inputs, rel):
    """1, tile - 1, tile, tile + 1 windows and the whole audio (438 windows, the last one partial)."""
    tile = amd_lib.whisper_amd_vad_tile()
    tag = "full" if rel == "full" else "c%d" % (1 if rel is None else tile + rel)
    g = G["front"][tag]
    check_front(vad.front(inputs[1][:g["n_samples"]]), g)


@pytest.mark.parametrize("slab", [100, 7])
def test_front_end_across_slabs(wrs, amd_lib, inputs, monkeypatch, slab):
    """438 windows in slabs of 100 (ragged last slab of 38) and of 7 (slabs that are no multiple of the tile)."""
    monkeypatch.setenv("WHISPER_AMD_VAD_SLAB", str(slab))
    v = wrs.WhisperVadContext.new(inputs[0], lib=amd_lib)
    try:
        check_front(v.front(inputs[1]), G["front"]["full"])
        assert bits(v.detect_speech(inputs[1])) == G["probs"]["full"]["bits"]
    finally:
        v.free()


def test_front_end_sizing_call(amd_lib, vad, inputs):
    pcm = np.ascontiguousarray(inputs[1][:1000])
    p = pcm.ctypes.data_as(C.POINTER(C.c_float))
    assert amd_lib.whisper_amd_vad_front(vad.ptr, p, 1000, None, 0) == 2 * 512
    out = np.full(600, np.float32(7.0))
    assert amd_lib.whisper_amd_vad_front(vad.ptr, p, 1000, out.ctypes.data_as(C.POINTER(C.c_float)), 520) == 2 * 512     # cap honoured
    assert (out[520:] == 7.0).all() and not (out[:520] == 7.0).all()


# ---- probabilities and segments ----
@pytest.mark.parametrize("tag", ["full", "n1", "n511", "n512", "n513"])
def test_probabilities_bit_exact(vad, inputs, tag):
    g = G["probs"][tag]
    got = vad.detect_speech(inputs[1][:g["n_samples"]])
    assert len(got) == -(-g["n_samples"] // 512)
    assert bits(got) == g["bits"]


def test_two_calls_in_a_row(vad, inputs):
    """The LSTM state is zeroed by every detect_speech call."""
    a = bits(vad.detect_speech(inputs[1]))
    vad.detect_speech(inputs[1][:513])
    assert bits(vad.detect_speech(inputs[1])) == a == G["probs"]["full"]["bits"]


def test_live_reference(wrs, vad, inputs):
    """Where the reference library is built: its probabilities and segments, now (otherwise the golden file has already said it)."""
    want, want_segs = G["probs"]["full"]["bits"], {t: G["segments"][t]["segments"] for t in V.PARAM_SETS}
    if os.path.exists(REF_LIB):
        ref = wrs.load_library(REF_LIB)
        wrs.set_log_callback(ref, None)
        r = wrs.WhisperVadContext.new(inputs[0], lib=ref)
        want = bits(r.detect_speech(inputs[1]))
        want_segs = {t: segs_int(r.segments_from_probs(wrs.vad_params(ref, *ps))) for t, ps in V.PARAM_SETS.items()}
        r.free()
    assert bits(vad.detect_speech(inputs[1])) == want
    for t, ps in V.PARAM_SETS.items():
        assert segs_int(vad.segments_from_probs(wrs.vad_params(vad.lib, *ps))) == want_segs[t]


@pytest.mark.parametrize("tag", list(V.PARAM_SETS))
def test_segments(wrs, vad, inputs, tag):
    p = wrs.vad_params(vad.lib, *V.PARAM_SETS[tag])
    vad.detect_speech(inputs[1])
    a = segs_int(vad.segments_from_probs(p))
    assert a == G["segments"][tag]["segments"]
    assert segs_int(vad.segments_from_samples(p, inputs[1])) == a


def test_default_params(wrs, amd_lib):
    p, c = amd_lib.whisper_vad_default_params(), amd_lib.whisper_vad_default_context_params()
    assert (p.threshold, p.min_speech_duration_ms, p.min_silence_duration_ms, p.speech_pad_ms) == (0.5, 250, 100, 30)
    assert p.max_speech_duration_s == np.finfo(np.float32).max and abs(p.samples_overlap - 0.1) < 1e-7
    assert (c.n_threads, c.use_gpu, c.gpu_device) == (4, False, 0)


# ---- results independent of the path ----
def test_loader_equals_file(wrs, amd_lib, inputs):
    v = wrs.WhisperVadContext.new_from_loader(open(inputs[0], "rb").read(), lib=amd_lib)
    try:
        assert bits(v.detect_speech(inputs[1])) == G["probs"]["full"]["bits"]
    finally:
        v.free()


def test_two_contexts_on_two_threads(wrs, amd_lib, inputs):
    ctxs = [wrs.WhisperVadContext.new(inputs[0], lib=amd_lib) for _ in range(2)]
    out, errs = [None, None], []

    def work(i):
        try:
            for _ in range(2):
                out[i] = bits(ctxs[i].detect_speech(inputs[1]))
        except Exception as e:     # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    [c.free() for c in ctxs]
    assert not errs
    assert out[0] == out[1] == G["probs"]["full"]["bits"]


def test_refused_models(wrs, amd_lib, tmp_path):
    logs = []
    wrs.set_log_callback(amd_lib, lambda lvl, txt: logs.append(txt))
    try:
        for name, data in {"bad_magic": V.model_bytes(magic=0x12345678), "wrong_layers": V.model_bytes(layers=[(129, 128), (128, 64), (64, 96), (96, 128)]),
                           "no_tensors": V.model_bytes(with_tensors=False), "truncated": V.model_bytes()[:200000]}.items():
            p = tmp_path / (name + ".bin")
            p.write_bytes(data)
            del logs[:]
            assert not amd_lib.whisper_vad_init_from_file_with_params(str(p).encode(), amd_lib.whisper_vad_default_context_params()), name
            if name != "bad_magic":
                assert "supported: n_window 512" in "".join(logs), name
        assert not amd_lib.whisper_vad_init_from_file_with_params(str(tmp_path / "absent.bin").encode(), amd_lib.whisper_vad_default_context_params())
    finally:
        import sys
        wrs.set_log_callback(amd_lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)


# ---- whisper_full(vad = true) ----
def full_ctx(wrs, amd_lib):
    return wrs.WhisperFullContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)


def vad_full_params(wrs, amd_lib, mp, **kw):
    return wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, vad=True, vad_model_path=mp, **kw)


def same(got, want, tokens=False):
    assert [(s["t0"], s["t1"], s["ids"]) for s in got] == [(s["t0"], s["t1"], s["ids"]) for s in want]
    if tokens:
        assert [(s["tok_t0"], s["tok_t1"]) for s in got] == [(s["tok_t0"], s["tok_t1"]) for s in want]


@pytest.fixture(scope="module")
def fctx(wrs, amd_lib):
    c = full_ctx(wrs, amd_lib)
    yield c
    c.free()


@pytest.mark.parametrize("tag", list(V.PARAM_SETS))
def test_full_with_vad(wrs, amd_lib, fctx, inputs, tag):
    fp = vad_full_params(wrs, amd_lib, inputs[0])
    fp.set("vad_params", wrs.vad_params(amd_lib, *V.PARAM_SETS[tag]))
    assert fctx.full(fp, inputs[1]) == 0
    got = fctx.segments()
    same(got, G["full"]["greedy_" + tag])
    assert got and got[0]["t0"] != 0                      # mapped back into the caller's audio


def test_full_with_vad_token_timestamps(wrs, amd_lib, fctx, inputs):
    assert fctx.full(vad_full_params(wrs, amd_lib, inputs[0], token_timestamps=True), inputs[1]) == 0
    same(fctx.segments(), G["full"]["greedy_token_timestamps"], tokens=True)


def test_full_with_vad_on_silence(wrs, amd_lib, fctx, inputs):
    assert fctx.full(vad_full_params(wrs, amd_lib, inputs[0]), inputs[1]) == 0 and fctx.segments()
    assert fctx.full(vad_full_params(wrs, amd_lib, inputs[0]), np.zeros(3 * SR, dtype=np.float32)) == 0
    assert fctx.segments() == []                          # whisper_full clears the earlier results


def test_full_with_wrong_vad_model_path(wrs, amd_lib, inputs, tmp_path):
    c = full_ctx(wrs, amd_lib)
    try:
        assert c.full(vad_full_params(wrs, amd_lib, str(tmp_path / "absent.bin")), inputs[1]) == -1
        assert c.full_parallel(vad_full_params(wrs, amd_lib, str(tmp_path / "absent.bin")), inputs[1], 2) == -1
    finally:
        c.free()


def test_full_parallel_with_vad(wrs, amd_lib, inputs):
    c = full_ctx(wrs, amd_lib)
    try:
        assert c.full_parallel(vad_full_params(wrs, amd_lib, inputs[0]), inputs[1], 2) == 0
        same(c.segments(), G["full"]["parallel2"])
        n = len(c.segments())
        assert c.full_parallel(vad_full_params(wrs, amd_lib, inputs[0]), np.zeros(3 * SR, dtype=np.float32), 2) == 0
        assert len(c.segments()) == n                     # no speech: 0, and unlike whisper_full the results stay
    finally:
        c.free()


def test_table_outlives_a_vad_off_call(wrs, amd_lib, inputs):
    """As in the reference: only the next VAD call on the state replaces the table; a vad = false call in between still maps through it."""
    c = full_ctx(wrs, amd_lib)
    try:
        assert c.full(vad_full_params(wrs, amd_lib, inputs[0]), inputs[1]) == 0
        assert c.full(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0), inputs[1][:SR * 6]) == 0
        same(c.segments(), G["full"]["then_vad_off_6s"])
    finally:
        c.free()


def test_vad_off_is_unmapped(wrs, amd_lib, inputs):
    """A fresh context with vad = false: plain times, the same through whisper_full and through whisper_full_with_state."""
    c = full_ctx(wrs, amd_lib)
    try:
        assert c.full(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0), inputs[1]) == 0
        got = c.segments()
        same(got, G["full"]["vad_off"])
    finally:
        c.free()
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    st = ctx.create_state()
    st.full(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, vad=True, vad_model_path=inputs[0]), inputs[1])     # whisper_full_with_state ignores vad
    assert [(s["t0"], s["t1"], s["ids"]) for s in st.segments()] == [(s["t0"], s["t1"], s["ids"]) for s in got]
    st.free()
    ctx.free()

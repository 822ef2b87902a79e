"""whisper_amd_full_long through the C ABI, on the s128 model, the synthetic VAD model and its 14 s audio.

A chunk is whisper_full_with_state on that chunk's speech-only audio, so everything here is an equality: one chunk is the reference engine's
recorded whisper_full(vad = true) result (tests/golden/vad.json); several chunks are, chunk by chunk, the plan of the issue's table, the
packed audio of tools/long_ref.py bit for bit, and the segments whisper_full_with_state gives on that audio alone on a fresh state - ids and
p / plog bit patterns - with times mapped by the test's own restatement of table and map_time (at least 10 cs, no overlap); where the live
reference library is built it transcribes each chunk's audio too.  The result does not depend on n_parallel, on the pack path, on where the
audio lies, or on the stalls of the chaos build."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import long_ref as R
import wsynth
import wsynth_vad as V
from conftest import GOLDEN, REF_LIB, ROOT

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLDEN, "vad.json")))
SR = 16000
OV = 0.1                            # whisper_vad_default_params().samples_overlap
SEGS = [tuple(s) for s in G["segments"]["default"]["segments"]]
PLANS = {                           # cap (ms) -> chunks (first, count, packed samples)
    30000: [(0, 3, 75360)],
    4000:  [(0, 2, 62400), (2, 1, 9760)],
    3500:  [(0, 1, 19360), (1, 2, 52800)],
    3000:  [(0, 1, 19360), (1, 1, 39840), (2, 1, 9760)],
}


def bits(x):
    return [int(v) for v in np.asarray(x, dtype=np.float32).view(np.uint32)]


def new_ctx(wrs, lib):
    return wrs.WhisperFullContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(lib, flash_attn=False), lib=lib)


def long_params(wrs, lib, mp=None, **kw):
    """greedy, best_of 1, no temperature fallback (as tests/test_vad_gpu.py); `vad` itself stays false: whisper_amd_full_long does not look at it"""
    return wrs.FullParams(lib, best_of=1, temperature_inc=0.0, vad_model_path=mp or V.model_path(), **kw)


def result(c):
    """every field of the context's result list that a chunk's own transcription determines"""
    out, lib = [], c.lib
    for i in range(lib.whisper_full_n_segments(c.ptr)):
        toks = [lib.whisper_full_get_token_data(c.ptr, i, j) for j in range(lib.whisper_full_n_tokens(c.ptr, i))]
        out.append(dict(t0=lib.whisper_full_get_segment_t0(c.ptr, i), t1=lib.whisper_full_get_segment_t1(c.ptr, i), ids=[t.id for t in toks],
                        p=bits([t.p for t in toks]), plog=bits([t.plog for t in toks]), tok_t0=[t.t0 for t in toks], tok_t1=[t.t1 for t in toks]))
    return out


def run_long(c, fp, pcm, cap, n_parallel=0):
    assert c.full_long(fp, pcm, cap, n_parallel) == 0
    return dict(segs=result(c), chunks=c.long_chunks(), pcm=[c.long_chunk_copy(i) for i in range(len(c.long_chunks()))], stats=c.long_stats(),
                batch=c.batch_stats())


@pytest.fixture(scope="module")
def pcm():
    return V.synth_audio()


@pytest.fixture(scope="module")
def fctx(wrs, amd_lib):
    c = new_ctx(wrs, amd_lib)
    yield c
    c.free()


@pytest.fixture(scope="module")
def runs(wrs, amd_lib, fctx, pcm):
    """whisper_amd_full_long once per cap of the table, default VAD parameters, n_parallel 8"""
    return {cap: run_long(fctx, long_params(wrs, amd_lib), pcm, cap) for cap in PLANS}


@pytest.fixture(scope="module")
def solo(wrs, amd_lib, pcm):
    """(first, count) -> whisper_full_with_state on the restated audio of that run of segments alone, each on a fresh state; computed once"""
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    out = {}
    for plan in PLANS.values():
        for first, count, _ in plan:
            for tts in (False, True):
                if (first, count, tts) in out or (tts and (first, count) not in [(f, k) for f, k, _ in PLANS[3000]]):
                    continue
                st = ctx.create_state()
                st.full(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, token_timestamps=tts), R.packed_audio(pcm, SEGS[first:first + count], OV))
                out[(first, count, tts)] = [dict(t0=s["t0"], t1=s["t1"], ids=s["ids"], p=bits(s["p"]), plog=bits(s["plog"]), tok_t0=s["tok_t0"],
                                                 tok_t1=s["tok_t1"]) for s in st.segments()]
                st.free()
    ctx.free()
    return out


def expected(plan, solo, tts=False):
    """the chunks' own results put together by the test's restatement of the mapping rules"""
    tables = [R.layout(SEGS[f:f + k], OV, G["n_samples"])[2] for f, k, _ in plan]
    res = [solo[(f, k, tts)] for f, k, _ in plan]
    times = R.map_segments([[(s["t0"], s["t1"]) for s in r] for r in res], tables)
    out = []
    for r, table in zip(res, tables):
        for s in r:
            t0, t1 = times[len(out)]
            out.append(dict(s, t0=t0, t1=t1, tok_t0=[R.map_time(t, table) if t >= 0 else t for t in s["tok_t0"]],
                            tok_t1=[R.map_time(t, table) if t >= 0 else t for t in s["tok_t1"]]))
    return out


# ---- one chunk: the reference engine's recorded whisper_full(vad = true) ----
@pytest.mark.parametrize("tag", list(V.PARAM_SETS))
def test_one_chunk_equals_the_reference(wrs, amd_lib, fctx, pcm, tag):
    fp = long_params(wrs, amd_lib)
    fp.set("vad_params", wrs.vad_params(amd_lib, *V.PARAM_SETS[tag]))
    assert fctx.full_long(fp, pcm, 30000, 8) == 0
    got = fctx.segments()
    assert [(s["t0"], s["t1"], s["ids"]) for s in got] == [(s["t0"], s["t1"], s["ids"]) for s in G["full"]["greedy_" + tag]]
    assert got and len(fctx.long_chunks()) == 1 and fctx.long_chunks()[0]["n_result"] == len(got)


# ---- several chunks ----
@pytest.mark.parametrize("cap", [3000, 3500, 4000])
def test_several_chunks(runs, solo, pcm, cap):
    r = runs[cap]
    assert [(c["first"], c["count"], c["packed"]) for c in r["chunks"]] == PLANS[cap]
    for c, got in zip(r["chunks"], r["pcm"]):
        want = R.packed_audio(pcm, SEGS[c["first"]:c["first"] + c["count"]], OV)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert (c["t0"], c["t1"]) == (SEGS[c["first"]][0], SEGS[c["first"] + c["count"] - 1][1])
        assert c["n_result"] == len(solo[(c["first"], c["count"], False)])
    want = expected(PLANS[cap], solo)
    assert len(want) >= len(PLANS[cap])                                   # every chunk of this audio says something
    assert r["segs"] == want
    assert all(b["t0"] >= a["t1"] for a, b in zip(want, want[1:])) and all(s["t1"] >= s["t0"] + 10 for s in want)
    assert r["stats"]["chunks"] == len(PLANS[cap]) and r["stats"]["waves"] == 1


def test_chunks_against_the_live_reference(wrs, solo, pcm):
    """Where the reference library is built: it transcribes each chunk's audio to the same ids and raw times."""
    if not os.path.exists(REF_LIB):
        pytest.skip("oracle/_ref/libwhisper_ref.so not built")
    ref = wrs.load_library(REF_LIB)
    wrs.set_log_callback(ref, None)
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(ref, use_gpu=False), lib=ref)
    for first, count, _ in PLANS[3000] + PLANS[3500][1:] + PLANS[4000][:1]:
        st = ctx.create_state()
        st.full(wrs.FullParams(ref, best_of=1, temperature_inc=0.0, n_threads=8), R.packed_audio(pcm, SEGS[first:first + count], OV))
        assert [(s["t0"], s["t1"], s["ids"]) for s in st.segments()] == [(s["t0"], s["t1"], s["ids"]) for s in solo[(first, count, False)]]
        st.free()
    ctx.free()


@pytest.mark.parametrize("n_parallel", [1, 2, 3, 8])
def test_n_parallel_does_not_change_the_result(wrs, amd_lib, fctx, runs, pcm, n_parallel):
    """3 chunks: three waves on the context's state alone, two waves (2 + 1: both member states used again, under lock step), one wave."""
    r = run_long(fctx, long_params(wrs, amd_lib), pcm, 3000, n_parallel)
    assert r["segs"] == runs[3000]["segs"]
    assert r["stats"]["waves"] == {1: 3, 2: 2}.get(n_parallel, 1)
    if n_parallel > 1:
        assert r["batch"][0] > 0 and r["batch"][1] >= r["batch"][0], "no lock-step passes formed: %r" % (r["batch"],)


@pytest.fixture(scope="module")
def solo_with_context(wrs, amd_lib, pcm):
    """as `solo` for the chunks of cap 3000, with no_context = false: on a fresh state there is no earlier text to carry"""
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    out = {}
    for first, count, _ in PLANS[3000]:
        st = ctx.create_state()
        st.full(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, no_context=False), R.packed_audio(pcm, SEGS[first:first + count], OV))
        out[(first, count, False)] = [dict(t0=s["t0"], t1=s["t1"], ids=s["ids"], p=bits(s["p"]), plog=bits(s["plog"]), tok_t0=s["tok_t0"],
                                           tok_t1=s["tok_t1"]) for s in st.segments()]
        st.free()
    ctx.free()
    return out


@pytest.mark.parametrize("n_parallel", [1, 2, 3])
def test_no_prompt_is_carried_between_chunks(wrs, amd_lib, pcm, solo_with_context, n_parallel):
    """no_context = false, after other calls on the same context: whisper_full keeps a state's text as the next call's prompt, and a member
    state runs one chunk per wave - yet every chunk must come out as it does alone on a fresh state, whatever ran on its state before
    (n_parallel 1: the context's state runs all three chunks; 2: it runs chunks 0 and 2; 3: chunk 0 only, after the earlier calls)."""
    want = expected(PLANS[3000], solo_with_context)
    c = new_ctx(wrs, amd_lib)
    try:
        assert c.full(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, no_context=False), pcm) == 0 and c.segments()      # text to carry
        assert c.full_long(long_params(wrs, amd_lib, no_context=False), pcm, 30000, n_parallel) == 0 and c.segments()
        r = run_long(c, long_params(wrs, amd_lib, no_context=False), pcm, 3000, n_parallel)
        assert r["segs"] == want
    finally:
        c.free()


def test_a_carried_prompt_would_show(wrs, amd_lib, pcm, solo_with_context):
    """The test above can fail: whisper_full_with_state twice on one state with no_context = false gives the first chunk another result
    the second time than on a fresh state."""
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    st = ctx.create_state()
    fp = wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, no_context=False)
    chunk = R.packed_audio(pcm, SEGS[0:1], OV)
    st.full(fp, R.packed_audio(pcm, SEGS[1:2], OV))
    st.full(fp, chunk)
    again = [(s["ids"], bits(s["p"])) for s in st.segments()]
    st.free()
    ctx.free()
    assert again != [(s["ids"], s["p"]) for s in solo_with_context[(0, 1, False)]]


def test_host_pack_path(wrs, amd_lib, fctx, runs, pcm, monkeypatch):
    assert runs[3000]["stats"]["path"] == 1 and runs[3000]["stats"]["fallbacks"] == 0
    monkeypatch.setenv("WHISPER_AMD_LONG_HOST", "1")
    r = run_long(fctx, long_params(wrs, amd_lib), pcm, 3000)
    assert r["stats"]["path"] == 0 and r["stats"]["fallbacks"] == 0
    assert r["segs"] == runs[3000]["segs"]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(r["pcm"], runs[3000]["pcm"]))
    monkeypatch.delenv("WHISPER_AMD_LONG_HOST")
    assert run_long(fctx, long_params(wrs, amd_lib), pcm, 3000)["stats"]["path"] == 1          # read at each call


def test_device_pointer_for_samples(wrs, amd_lib, fctx, runs, pcm):
    assert runs[3000]["stats"]["h2d_bytes"] == 4 * len(pcm)               # host PCM: one upload
    st = wrs.WhisperState(fctx, fctx.state_ptr())
    ptr, n = st.audio_to_pcm(pcm, 1, 16000)
    r = run_long(fctx, long_params(wrs, amd_lib), (ptr, n), 3000)
    assert r["stats"]["h2d_bytes"] == 0 and r["stats"]["path"] == 1
    assert r["segs"] == runs[3000]["segs"]


def stereo_i16(x, seed):
    """a fixed int16 stereo recording of a mono F32 signal (|x| <= 0.5): the channels differ by seeded noise and average to the signal at 16 bits,
    so the VAD hears what it hears in the signal itself"""
    rng = np.random.default_rng(seed)
    base, d = np.rint(x.astype(np.float64) * 32768.0), rng.integers(-40, 41, len(x))
    return np.stack([base + d, base - d], axis=1).astype(np.int16).reshape(-1)


def test_full_long_audio(wrs, amd_lib, fctx, pcm):
    fp = long_params(wrs, amd_lib)
    x = stereo_i16(pcm, 31)
    assert fctx.full_long_audio(fp, x, 2, 16000, max_chunk_ms=3000) == 0
    a, a_chunks = result(fctx), fctx.long_chunks()
    assert fctx.long_stats()["h2d_bytes"] == 0                            # the PCM itself never crossed: only the int16 recording did
    assert fctx.full_long(fp, wrs.convert_stereo_i16_to_mono_f32(x), 3000) == 0
    assert a and a == result(fctx) and a_chunks == fctx.long_chunks() and len(a_chunks) > 1
    # 44.1 kHz mono F32: the front end's own 16 kHz result, read back, through whisper_amd_full_long
    up = np.interp(np.arange(len(pcm) * 441 // 160) * (160.0 / 441.0), np.arange(len(pcm)), pcm).astype(np.float32)
    assert fctx.full_long_audio(fp, up, 1, 44100, max_chunk_ms=3000) == 0
    b, b_chunks = result(fctx), fctx.long_chunks()
    down = wrs.WhisperState(fctx, fctx.state_ptr()).audio_copy()
    assert abs(len(down) - len(pcm)) <= 1
    assert fctx.full_long(fp, down, 3000) == 0
    assert b and b == result(fctx) and b_chunks == fctx.long_chunks()


def test_token_timestamps(wrs, amd_lib, fctx, solo, pcm):
    r = run_long(fctx, long_params(wrs, amd_lib, token_timestamps=True), pcm, 3000, 3)
    want = expected(PLANS[3000], solo, tts=True)
    assert r["segs"] == want
    assert any(t >= 0 for s in want for t in s["tok_t0"]) and want[0]["tok_t0"] != solo[(0, 1, True)][0]["tok_t0"]       # set, and mapped


# ---- edges ----
def test_silence_gives_no_segments(wrs, amd_lib, fctx, pcm):
    assert fctx.full_long(long_params(wrs, amd_lib), pcm, 3000) == 0 and fctx.segments()
    assert fctx.full_long(long_params(wrs, amd_lib), np.zeros(3 * SR, dtype=np.float32), 3000) == 0
    assert fctx.segments() == [] and fctx.long_chunks() == []             # earlier results are cleared, as whisper_full does


def test_refusals(wrs, amd_lib, pcm, tmp_path):
    c = new_ctx(wrs, amd_lib)
    try:
        assert c.full_long(long_params(wrs, amd_lib, mp=str(tmp_path / "absent.bin")), pcm, 3000) == -1
        assert c.full_long(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0), pcm, 3000) == -1           # no VAD model path at all
        assert c.full_long(long_params(wrs, amd_lib, offset_ms=10), pcm, 3000) == -1
        assert c.full_long(long_params(wrs, amd_lib, duration_ms=1000), pcm, 3000) == -1
        assert amd_lib.whisper_amd_full_long(c.ptr, long_params(wrs, amd_lib).c, None, 100, 0, 0) == -1
        assert amd_lib.whisper_amd_full_long(None, long_params(wrs, amd_lib).c, None, 100, 0, 0) == -1
        assert c.segments() == []
        assert c.full_long(long_params(wrs, amd_lib), pcm, 3000) == 0 and c.segments() and len(c.long_chunks()) == 3
        bad = wrs.FullParams(amd_lib, best_of=9, temperature_inc=0.0, vad_model_path=V.model_path())       # more decoders than whisper_full takes: every chunk returns -4
        assert c.full_long(bad, pcm, 3000) == -4
        assert c.segments() == [] and c.long_chunks() == []                 # a failed call leaves neither results nor chunks
        assert c.full_long(long_params(wrs, amd_lib), pcm, 0, 0) == 0 and len(c.long_chunks()) == 1          # the defaults: 30 s, 8 members
    finally:
        c.free()


def test_last_segment_reaches_the_end(wrs, amd_lib, fctx, pcm):
    """The audio cut at 9.0 s, inside the 7.0 - 9.5 s burst: the last segment ends with the audio (the one-sample rule).  One chunk is then
    the product's own whisper_full(vad = true), and the live reference's where it is built."""
    cut = pcm[:9 * SR]
    assert fctx.full_long(long_params(wrs, amd_lib), cut, 30000) == 0
    got = [(s["t0"], s["t1"], s["ids"]) for s in fctx.segments()]
    ch = fctx.long_chunks()
    assert len(ch) == 1 and R.cs_to_samples(ch[0]["t1"]) >= len(cut) - 1
    c = new_ctx(wrs, amd_lib)
    try:
        assert c.full(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, vad=True, vad_model_path=V.model_path()), cut) == 0
        assert got and got == [(s["t0"], s["t1"], s["ids"]) for s in c.segments()]
    finally:
        c.free()
    if os.path.exists(REF_LIB):
        ref = wrs.load_library(REF_LIB)
        wrs.set_log_callback(ref, None)
        r = wrs.WhisperFullContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(ref, use_gpu=False), lib=ref)
        try:
            assert r.full(wrs.FullParams(ref, best_of=1, temperature_inc=0.0, vad=True, vad_model_path=V.model_path(), n_threads=8), cut) == 0
            assert got == [(s["t0"], s["t1"], s["ids"]) for s in r.segments()]
        finally:
            r.free()


def test_two_calls_in_a_row(wrs, amd_lib, pcm, runs):
    c = new_ctx(wrs, amd_lib)
    try:
        a = run_long(c, long_params(wrs, amd_lib), pcm, 3000)
        assert a["segs"] == runs[3000]["segs"] and len(a["chunks"]) == 3
        b = run_long(c, long_params(wrs, amd_lib), pcm, 4000)
        assert b["segs"] == runs[4000]["segs"] and b["chunks"] == runs[4000]["chunks"] and len(b["chunks"]) == 2
        assert amd_lib.whisper_amd_long_n_chunks(c.ptr) == 2 and amd_lib.whisper_amd_long_chunk_info(c.ptr, 2, (C.c_int64 * 6)()) == -1
        assert amd_lib.whisper_amd_long_chunk_copy(c.ptr, 2, None, 0) == -1
        again = run_long(c, long_params(wrs, amd_lib), pcm, 4000)
        assert again["segs"] == b["segs"] and again["chunks"] == b["chunks"]
    finally:
        c.free()


def test_new_segment_callback_and_language(wrs, amd_lib, fctx, runs, pcm):
    """new_segment_callback fires on the context's state once per appended segment, with the list as long as it is at that moment."""
    seen = []
    fp = long_params(wrs, amd_lib)
    fp.set("new_segment_callback", lambda ctx, st, n_new, ud: seen.append((st, n_new, amd_lib.whisper_full_n_segments_from_state(st))))
    assert fctx.full_long(fp, pcm, 3000, 3) == 0
    n = len(runs[3000]["segs"])
    assert seen == [(fctx.state_ptr(), 1, i + 1) for i in range(n)]
    assert amd_lib.whisper_full_lang_id_from_state(fctx.state_ptr()) == 0


def test_chaos_build(wrs, runs, pcm):
    """libwhisper_chaos.so - the one-launch steps with random stalls in front of their products: the same segments."""
    path = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(path)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    c = new_ctx(wrs, lib)
    try:
        assert run_long(c, long_params(wrs, lib), pcm, 3000, 3)["segs"] == runs[3000]["segs"]
    finally:
        c.free()

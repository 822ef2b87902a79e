"""whisper_amd_full_long_channels and whisper_amd_channel_speakers through the C ABI, on the s128 model and the synthetic VAD model.

The yardstick, stated once: with the gate off, the segments of channel c in the merged list are exactly what whisper_amd_full_long gives on
whisper_amd_audio_to_pcm of channel c extracted on the host - texts, token ids, p / plog bit patterns, t0 / t1 and token times - whichever chunks
shared a lock-step pass.  The recordings are tools/channels_cases.py's: two_speakers (3 + 3 VAD segments whose times differ and overlap across the
channels; 3 + 3 chunks at a cap of 3000 ms), as F32 at 16 kHz and as int16 at 8 kHz; bleed (channel 1 = 0.8 x channel 0 plus a burst of its
own: BLEED = 0.8 is the factor at which the reference VAD, run on the CPU when the fixture was chosen, still finds the three bled segments;
the gate runs at g = 0.9, between it and 1); alternating (the speakers take turns; the down-mix is the VAD audio)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

import channels_cases as K
import wsynth
import wsynth_vad as V
from conftest import ROOT

pytestmark = pytest.mark.gpu

I16, F32 = 0, 1
GATE = 0.9


def bits(x):
    return [int(v) for v in np.asarray(x, dtype=np.float32).view(np.uint32)]


def new_ctx(wrs, lib):
    return wrs.WhisperFullContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(lib, flash_attn=False), lib=lib)


def long_params(wrs, lib, mp=None, **kw):
    return wrs.FullParams(lib, best_of=1, temperature_inc=0.0, vad_model_path=mp or V.model_path(), **kw)


def result(c):
    out, lib = [], c.lib
    for i in range(lib.whisper_full_n_segments(c.ptr)):
        toks = [lib.whisper_full_get_token_data(c.ptr, i, j) for j in range(lib.whisper_full_n_tokens(c.ptr, i))]
        out.append(dict(t0=lib.whisper_full_get_segment_t0(c.ptr, i), t1=lib.whisper_full_get_segment_t1(c.ptr, i),
                        text=lib.whisper_full_get_segment_text(c.ptr, i), ids=[t.id for t in toks], p=bits([t.p for t in toks]),
                        plog=bits([t.plog for t in toks]), tok_t0=[t.t0 for t in toks], tok_t1=[t.t1 for t in toks], tok_dtw=[t.t_dtw for t in toks]))
    return out


def run_channels(c, fp, data, rate, cap, n_parallel=0, g=0.0, fmt=None):
    assert c.full_long_channels(fp, data, rate, fmt, cap, n_parallel, g) == 0
    return dict(segs=result(c), ch=c.segment_channels(), chunks=c.long_chunks(), chunk_ch=c.chunk_channels(), stats=c.channels_stats(),
                lstats=c.long_stats())


def of_channel(r, ch):
    return [s for s, k in zip(r["segs"], r["ch"]) if k == ch]


class DeviceCopy:
    def __init__(self, x):
        self.hip = C.CDLL("libamdhip64.so")
        self.base = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.base), C.c_size_t(x.nbytes + 256)) == 0
        self.ptr = self.base.value
        assert self.hip.hipMemcpy(C.c_void_p(self.ptr), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0

    def free(self):
        self.hip.hipFree(self.base)


@pytest.fixture(scope="module")
def recs():
    x = K.two_speakers()
    return {"f32_16k": (x, 16000), "i16_8k": (K.at_8k_i16(x), 8000)}


@pytest.fixture(scope="module")
def fctx(wrs, amd_lib):
    c = new_ctx(wrs, amd_lib)
    yield c
    c.free()


@pytest.fixture(scope="module")
def runs(wrs, amd_lib, fctx, recs):
    """whisper_amd_full_long_channels once per recording and cap, gate off, n_parallel 8"""
    return {(tag, cap): run_channels(fctx, long_params(wrs, amd_lib), x, rate, cap) for tag, (x, rate) in recs.items() for cap in (30000, 3000)}


@pytest.fixture(scope="module")
def yard(wrs, amd_lib, recs):
    """(recording, cap, channel) -> whisper_amd_full_long on whisper_amd_audio_to_pcm of that channel extracted on the host; computed once"""
    c = new_ctx(wrs, amd_lib)
    st = wrs.WhisperState(c, c.state_ptr())
    out = {}
    for tag, (x, rate) in recs.items():
        for ch in (0, 1):
            for cap in (30000, 3000):
                ptr, n = st.audio_to_pcm(K.channel(x, ch), 1, rate)
                assert c.full_long(long_params(wrs, amd_lib), (ptr, n), cap) == 0
                out[(tag, cap, ch)] = dict(segs=result(c), stats=c.long_stats(), chunks=c.long_chunks())
                assert c.segment_channels() == [-1] * len(out[(tag, cap, ch)]["segs"])      # a plain long call has no channels
    c.free()
    return out


# ---- the yardstick ----
@pytest.mark.parametrize("cap", [30000, 3000])
@pytest.mark.parametrize("tag", ["f32_16k", "i16_8k"])
def test_each_channel_is_its_own_full_long(runs, yard, tag, cap):
    """Observed once, in the first GPU run of this file: [i16_8k-3000] differed in the second segment of channel 1 (the 2.5 s chunk, fourth of
    six in its wave).  The same calls in the same order gave equal results in every later run (seven, the whole suite among them); the cause was not found."""
    r = runs[(tag, cap)]
    for ch in (0, 1):
        want = yard[(tag, cap, ch)]["segs"]
        assert want, "the yardstick said nothing on channel %d" % ch
        assert of_channel(r, ch) == want
    assert len(r["segs"]) == sum(len(yard[(tag, cap, ch)]["segs"]) for ch in (0, 1)) and set(r["ch"]) == {0, 1}


def test_one_wave_instead_of_two(wrs, amd_lib, fctx, runs, yard, recs):
    r = runs[("f32_16k", 3000)]
    c0, c1 = (len(yard[("f32_16k", 3000, ch)]["chunks"]) for ch in (0, 1))
    assert c0 >= 2 and c1 >= 2 and c0 + c1 <= 8
    assert r["stats"]["chunks"] == c0 + c1 == len(r["chunks"]) and r["stats"]["waves"] == 1
    assert all(yard[("f32_16k", 3000, ch)]["stats"]["waves"] == 1 for ch in (0, 1))         # two plain calls: a wave each
    x, rate = recs["f32_16k"]
    two = run_channels(fctx, long_params(wrs, amd_lib), x, rate, 3000, n_parallel=2)
    assert two["stats"]["waves"] == math.ceil((c0 + c1) / 2) and two["stats"]["chunks"] == c0 + c1
    assert two["segs"] == r["segs"] and two["ch"] == r["ch"]


def test_stats_and_device_input(wrs, amd_lib, fctx, runs, recs):
    for (tag, cap), r in runs.items():
        s = r["stats"]
        assert (s["split_path"], s["split_fallbacks"], s["energy_launches"], s["pack_launches"], s["dropped"]) == (1, 0, 0, 1, 0), (tag, cap, s)
        assert s["energy_fallbacks"] == 0
        assert s["h2d_bytes"] == recs[tag][0].nbytes                    # the recording crossed once
        assert s["segments_0"] >= 2 and s["segments_1"] >= 2
    x, rate = recs["i16_8k"]
    d = DeviceCopy(x)
    try:
        r = run_channels(fctx, long_params(wrs, amd_lib), (d.ptr, len(x) // 2), rate, 3000, fmt=I16)
    finally:
        d.free()
    assert r["stats"]["h2d_bytes"] == 0 and r["stats"]["split_path"] == 1 and r["stats"]["pack_launches"] == 1
    assert r["segs"] == runs[("i16_8k", 3000)]["segs"] and r["ch"] == runs[("i16_8k", 3000)]["ch"]


@pytest.mark.parametrize("cap", [30000, 3000])
def test_merged_order_and_clamps(runs, yard, cap):
    r = runs[("f32_16k", cap)]
    t0 = [s["t0"] for s in r["segs"]]
    assert t0 == sorted(t0)
    for ch in (0, 1):
        mine = of_channel(r, ch)
        assert all(b["t0"] >= a["t1"] for a, b in zip(mine, mine[1:])) and all(s["t1"] >= s["t0"] + 10 for s in mine)
    assert any(a["t0"] < b["t1"] and b["t0"] < a["t1"] for a in of_channel(r, 0) for b in of_channel(r, 1)), "no overlap across the channels survived"
    # the two lists differ, and the chunks are in wave order: (original start, channel)
    assert [(s["t0"], s["t1"]) for s in of_channel(r, 0)] != [(s["t0"], s["t1"]) for s in of_channel(r, 1)]
    order = [(c["t0"], k) for c, k in zip(r["chunks"], r["chunk_ch"])]
    assert order == sorted(order) and set(r["chunk_ch"]) == {0, 1}
    for ch in (0, 1):
        assert [c for c, k in zip(r["chunks"], r["chunk_ch"]) if k == ch] == yard[("f32_16k", cap, ch)]["chunks"]


def test_channel_getters_after_a_plain_call(wrs, amd_lib, fctx, recs):
    x, rate = recs["f32_16k"]
    r = run_channels(fctx, long_params(wrs, amd_lib), x, rate, 3000)
    n = len(r["segs"])
    assert amd_lib.whisper_amd_long_segment_channel(fctx.ptr, n) == -1 and amd_lib.whisper_amd_long_segment_channel(fctx.ptr, -1) == -1
    assert amd_lib.whisper_amd_long_chunk_channel(fctx.ptr, len(r["chunks"])) == -1
    assert fctx.full_long(long_params(wrs, amd_lib), K.channel(x, 0), 3000) == 0 and fctx.segments()
    assert set(fctx.segment_channels()) == {-1} and set(fctx.chunk_channels()) == {-1}


def test_new_segment_callback_and_language(wrs, amd_lib, fctx, runs, recs):
    seen = []
    fp = long_params(wrs, amd_lib)
    fp.set("new_segment_callback", lambda ctx, st, n_new, ud: seen.append((st, n_new, amd_lib.whisper_full_n_segments_from_state(st))))
    x, rate = recs["f32_16k"]
    assert fctx.full_long_channels(fp, x, rate, None, 3000, 3) == 0
    assert seen == [(fctx.state_ptr(), 1, i + 1) for i in range(len(runs[("f32_16k", 3000)]["segs"]))]
    assert amd_lib.whisper_full_lang_id_from_state(fctx.state_ptr()) == 0


# ---- silent channels ----
def test_one_silent_channel_and_both(wrs, amd_lib, fctx, runs, recs):
    x, rate = recs["f32_16k"]
    y = x.copy()
    y[1::2] = 0.0
    r = run_channels(fctx, long_params(wrs, amd_lib), y, rate, 3000)
    assert r["segs"] == of_channel(runs[("f32_16k", 3000)], 0) and set(r["ch"]) == {0} and set(r["chunk_ch"]) == {0}
    assert r["stats"]["segments_1"] == 0 and r["stats"]["segments_0"] == runs[("f32_16k", 3000)]["stats"]["segments_0"]
    z = x.copy()
    z[0::2] = 0.0
    r = run_channels(fctx, long_params(wrs, amd_lib), z, rate, 3000)
    assert r["segs"] == of_channel(runs[("f32_16k", 3000)], 1) and set(r["ch"]) == {1}
    r = run_channels(fctx, long_params(wrs, amd_lib), np.zeros(2 * 3 * 16000, np.float32), rate, 3000)
    assert r["segs"] == [] and r["chunks"] == [] and r["ch"] == []          # earlier results are cleared, as whisper_full does
    assert (r["stats"]["segments_0"], r["stats"]["segments_1"], r["stats"]["chunks"], r["stats"]["waves"], r["stats"]["pack_launches"]) == (0, 0, 0, 0, 0)


# ---- the gate ----
def test_crosstalk_gate(wrs, amd_lib, fctx):
    x = K.bleed()
    lo, hi = (int(100 * t) for t in K.OWN_BURST)
    off = run_channels(fctx, long_params(wrs, amd_lib), x, 16000, 3000)
    assert off["stats"]["energy_launches"] == 0 and off["stats"]["dropped"] == 0
    assert off["stats"]["segments_1"] == off["stats"]["segments_0"] + 1          # the VAD hears the bleed: every segment of channel 0, and the burst
    bled = [s for s in of_channel(off, 1) if s["t0"] < lo - 20]
    assert bled, "the bled segments were not transcribed with the gate off"
    on = run_channels(fctx, long_params(wrs, amd_lib), x, 16000, 3000, g=GATE)
    assert K.BLEED < GATE < 1.0
    assert on["stats"]["energy_launches"] == 1 and on["stats"]["pack_launches"] == 1 and on["stats"]["energy_fallbacks"] == 0
    assert on["stats"]["dropped"] == off["stats"]["segments_0"] and on["stats"]["segments_1"] == off["stats"]["segments_1"]
    mine = [(c["t0"], c["t1"]) for c, k in zip(on["chunks"], on["chunk_ch"]) if k == 1]
    assert len(mine) == 1 and lo - 20 <= mine[0][0] and mine[0][1] <= hi + 20       # only the own burst remains on channel 1
    assert of_channel(on, 1) and all(lo - 20 <= s["t0"] and s["t1"] <= hi + 20 for s in of_channel(on, 1))
    assert of_channel(on, 0) == of_channel(off, 0) and of_channel(on, 0)
    assert fctx.full_long_channels(long_params(wrs, amd_lib), x, 16000, None, 3000, 0, -0.5) == -1        # a negative ratio is refused


# ---- the cli's --diarize rule ----
def test_channel_speakers_on_a_down_mixed_run(wrs, amd_lib, fctx):
    x = K.alternating()
    assert fctx.full_long_audio(long_params(wrs, amd_lib), x, 2, 16000, max_chunk_ms=3000) == 0
    times = [(s["t0"], s["t1"]) for s in result(fctx)]
    assert len(times) >= 2
    st = wrs.WhisperState(fctx, fctx.state_ptr())
    ptr, n, stride = st.audio_split(x, 16000)
    assert n == len(x) // 2 and stride % 64 == 0 and 0 <= stride - n < 64
    planes = [st.audio_split_copy(c) for c in (0, 1)]
    assert all(np.array_equal(planes[c], K.channel(x, c)) for c in (0, 1))
    labels, e = st.channel_speakers(times)
    want = []
    for i, (t0, t1) in enumerate(times):
        is0, is1 = (max(0, min(n - 1, int(t * 16000 / 100))) for t in (t0, t1))            # examples/common-whisper.cpp: timestamp_to_sample
        e0, e1 = (float(np.cumsum(np.abs(p[is0:is1]).astype(np.float64))[-1]) if is1 > is0 else 0.0 for p in planes)      # the cli's sequential sums
        tol = (is1 - is0) * 2.0 ** -53
        assert abs(e[i, 0] - e0) <= tol * e0 and abs(e[i, 1] - e1) <= tol * e1
        assert abs(e0 - 1.1 * e1) > 1e-6 * e0 and abs(e1 - 1.1 * e0) > 1e-6 * e1               # no summation order decides this label
        want.append(0 if e0 > 1.1 * e1 else 1 if e1 > 1.1 * e0 else -1)
    assert list(labels) == want and {0, 1} <= set(want)
    assert list(st.channel_speakers(times, 1e6)[0]) == [-1] * len(times)                       # no speaker is a million times louder
    # the host function and the kernel agree bit for bit on these spans
    spans = [(max(0, min(n - 1, int(t0 * 160))), max(0, min(n - 1, int(t1 * 160)))) for t0, t1 in times] + [(0, n), (5, 5), (-3, 2)]
    a, b = st.channel_energy(spans, 0), st.channel_energy(spans, 1)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.all(a[-2] == 0.0)
    assert amd_lib.whisper_amd_channel_speakers(fctx.state_ptr(), None, None, 2, 0.0, None, None) == -1
    fresh = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, gpu_device=0), lib=amd_lib)
    s2 = fresh.create_state()
    assert amd_lib.whisper_amd_audio_split_copy(s2.ptr, 0, None, 0) == -1                      # no split yet
    assert amd_lib.whisper_amd_channel_energy(s2.ptr, None, None, 0, 1, None) == -1
    s2.free()
    fresh.free()


# ---- robustness ----
def test_host_path(wrs, amd_lib, fctx, runs, recs, monkeypatch):
    x, rate = recs["i16_8k"]
    monkeypatch.setenv("WHISPER_AMD_CHANNELS_HOST", "1")
    r = run_channels(fctx, long_params(wrs, amd_lib), x, rate, 3000)
    assert r["stats"]["split_path"] == 0 and r["stats"]["split_fallbacks"] == 0
    assert r["segs"] == runs[("i16_8k", 3000)]["segs"] and r["ch"] == runs[("i16_8k", 3000)]["ch"]
    g = run_channels(fctx, long_params(wrs, amd_lib), K.bleed(), 16000, 3000, g=GATE)
    assert g["stats"]["energy_launches"] == 0 and g["stats"]["dropped"] == g["stats"]["segments_0"]        # the gate through the host function
    monkeypatch.delenv("WHISPER_AMD_CHANNELS_HOST")
    assert run_channels(fctx, long_params(wrs, amd_lib), x, rate, 3000)["stats"]["split_path"] == 1        # read at each call
    monkeypatch.setenv("WHISPER_AMD_LONG_HOST", "1")
    r = run_channels(fctx, long_params(wrs, amd_lib), x, rate, 3000)
    assert r["stats"]["pack_launches"] == 0 and r["lstats"]["path"] == 0 and r["segs"] == runs[("i16_8k", 3000)]["segs"]


def test_two_calls_in_a_row(wrs, amd_lib, runs, recs):
    c = new_ctx(wrs, amd_lib)
    try:
        x, rate = recs["f32_16k"]
        a = run_channels(c, long_params(wrs, amd_lib), x, rate, 3000)
        b = run_channels(c, long_params(wrs, amd_lib), x, rate, 30000)
        again = run_channels(c, long_params(wrs, amd_lib), recs["i16_8k"][0], 8000, 3000)
        assert (a["segs"], a["ch"]) == (runs[("f32_16k", 3000)]["segs"], runs[("f32_16k", 3000)]["ch"])
        assert (b["segs"], b["chunks"]) == (runs[("f32_16k", 30000)]["segs"], runs[("f32_16k", 30000)]["chunks"])
        assert again["segs"] == runs[("i16_8k", 3000)]["segs"]
    finally:
        c.free()


def test_refusals(wrs, amd_lib, recs, tmp_path):
    c = new_ctx(wrs, amd_lib)
    try:
        x, rate = recs["f32_16k"]
        lib, fp = amd_lib, long_params(wrs, amd_lib)
        # a missing or absent VAD model fails inside the call (a context keeps the VAD context its first call made: these come first): results
        # and chunks are cleared, as whisper_amd_full_long clears them
        assert c.full(wrs.FullParams(lib, best_of=1, temperature_inc=0.0), K.channel(x, 0)) == 0 and c.segments()
        assert c.full_long_channels(long_params(wrs, lib, mp=str(tmp_path / "absent.bin")), x, rate, None, 3000) == -1
        assert c.segments() == [] and c.long_chunks() == [] and c.segment_channels() == []
        assert c.full_long_channels(wrs.FullParams(lib, best_of=1, temperature_inc=0.0), x, rate, None, 3000) == -1          # no VAD model path at all
        good = run_channels(c, fp, x, rate, 3000)
        cp = wrs.whisper_amd_channels_params()
        lib.whisper_amd_channels_default_params(C.byref(cp))
        assert (cp.max_chunk_ms, cp.n_parallel, cp.crosstalk_ratio) == (30000, 8, 0.0)
        data, nf = C.c_void_p(x.ctypes.data), len(x) // 2
        bad = [(c.ptr, fp, C.byref(cp), None, nf, rate, F32), (None, fp, C.byref(cp), data, nf, rate, F32), (c.ptr, fp, None, data, nf, rate, F32),
               (c.ptr, fp, C.byref(cp), data, -1, rate, F32), (c.ptr, fp, C.byref(cp), data, 0, rate, F32), (c.ptr, fp, C.byref(cp), data, nf, 7999, F32),
               (c.ptr, fp, C.byref(cp), data, nf, 16001, F32), (c.ptr, fp, C.byref(cp), data, nf, rate, 2),
               (c.ptr, long_params(wrs, lib, offset_ms=10), C.byref(cp), data, nf, rate, F32),
               (c.ptr, long_params(wrs, lib, duration_ms=1000), C.byref(cp), data, nf, rate, F32)]
        for ctx_p, p, cpp, d, n, r, f in bad:
            assert lib.whisper_amd_full_long_channels(ctx_p, p.c, cpp, d, n, r, f) == -1, (n, r, f)
        cp.crosstalk_ratio = -1.0
        assert lib.whisper_amd_full_long_channels(c.ptr, fp.c, C.byref(cp), data, nf, rate, F32) == -1
        # refused before anything was touched, as whisper_amd_full_long's own refusals: the earlier results stand
        assert result(c) == good["segs"] and c.segment_channels() == good["ch"] and c.long_chunks() == good["chunks"]
        n64, s64 = C.c_int64(-77), C.c_int64(-78)
        st = c.state_ptr()
        for d, n, r, f in [(None, 10, rate, F32), (data, -1, rate, F32), (data, 100, 7999, F32), (data, 100, 192001, I16), (data, 100, rate, -1)]:
            assert not lib.whisper_amd_audio_split(st, d, n, r, f, C.byref(n64), C.byref(s64)) and (n64.value, s64.value) == (-77, -78)
        assert not lib.whisper_amd_audio_split(None, data, 100, rate, F32, C.byref(n64), C.byref(s64))
        assert not lib.whisper_amd_audio_split(st, data, 100, rate, F32, None, C.byref(s64))
        too_many = wrs.FullParams(lib, best_of=9, temperature_inc=0.0, vad_model_path=V.model_path())       # every chunk returns -4
        assert c.full_long_channels(too_many, x, rate, None, 3000) == -4
        assert c.segments() == [] and c.long_chunks() == []
        dflt = run_channels(c, fp, x, rate, 0, 0)                                                           # the defaults: 30 s, 8 members
        assert dflt["stats"]["chunks"] == 2 and dflt["stats"]["waves"] == 1
    finally:
        c.free()


def test_chaos_build(wrs, runs, recs):
    """libwhisper_chaos.so - the one-launch steps with random stalls in front of their products: the same segments."""
    path = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(path)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    c = new_ctx(wrs, lib)
    try:
        x, rate = recs["f32_16k"]
        r = run_channels(c, long_params(wrs, lib), x, rate, 3000, 3)
        assert r["segs"] == runs[("f32_16k", 3000)]["segs"] and r["ch"] == runs[("f32_16k", 3000)]["ch"]
    finally:
        c.free()

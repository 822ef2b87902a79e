"""Live streaming sessions end to end (whisper_amd_stream_*), model s128, audio wsynth.synth_audio.

The yardstick is tools/stream_ref.py, the literal restatement of the reference's examples/stream/stream.cpp: its pcmf32 and prompt_tokens of
every iteration.  A session's window PCM and prompt must equal them bit for bit, and its segments (ids, text, p, plog) those of a second
product state that runs full() on the restatement's windows and prompts, and those the reference engine gave (tests/golden/s128_stream.json,
written by tools/gen_golden_stream.py on the CPU).  Packet size, input rate and format, the number of sessions stepped together, the host
path and the stalls of the chaos build must not change a result."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, GOLDEN

import wsynth
import gen_golden_stream as GG
from stream_ref import StreamRef, drive

pytestmark = pytest.mark.gpu

A, B = "greedy_1000_4000_200", "beam3_3000_6000_200"
I16, F32 = 0, 1


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def segs_of(state):
    return [dict(text=s["text"].decode("latin1"), ids=s["ids"], p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]])
            for s in state.segments()]


def stream_kw(name, **kw):
    step, length, keep = GG.CONFIGS[name][0]
    return dict(dict(step_ms=step, length_ms=length, keep_ms=keep), **kw)


def run_session(wrs, lib, s, name, audio, packet, channels=1, after=None, flush=False):
    """feed `audio` (frames x channels, interleaved) in packets of `packet` frames (an int or a list); step whenever a window is due"""
    fp = GG.full_params(lib, name, None)
    out = []
    sizes = packet if isinstance(packet, list) else [packet] * (len(audio) // channels // packet)

    def drain():
        while s.pending() > 0:
            assert s.step(fp) == 1
            out.append(dict(pcm=s.window(), prompt=s.prompt(), segs=segs_of(s.state), info=s.info()))
            if after:
                after(out[-1])

    at = 0
    for n in sizes:
        due = s.feed(audio[at * channels:(at + n) * channels])
        assert due >= 0 and due == s.pending(), due
        at += n
        drain()
    if flush:
        assert s.flush() == s.pending()
        drain()
    assert s.step(fp) == 0
    return out


def check_against(windows, want, z):
    """a session's windows against the restatement's records; info against the plan"""
    assert len(windows) == len(want)
    for k, (w, r) in enumerate(zip(windows, want)):
        assert w["pcm"].shape == r["pcm"].shape and np.array_equal(bits(w["pcm"]), bits(r["pcm"])), ("window PCM", k)
        assert w["prompt"] == r["prompt"], ("prompt", k)
        assert w["segs"] == r["segs"], ("segments", k)
        i = w["info"]
        assert (i["windows"], i["length"], i["take"], i["committed"], i["prompt_tokens"], i["dropped"]) == \
               (k + 1, len(r["pcm"]), r["take"], 1 if r["committed"] else 0, len(r["prompt"]), 0), (k, i)
        assert i["start"] == (k + 1) * z.n_samples_step - len(r["pcm"]) and i["feeds_host"] == 0 and i["feeds_device"] > 0


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "s128_stream.json")))


@pytest.fixture(scope="module")
def audio(golden):
    return wsynth.synth_audio(16000 * golden["seconds"], golden["audio_seed"])


@pytest.fixture(scope="module")
def ctx(wrs, amd_lib):
    c = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    yield c
    c.free()


def restated(wrs, lib, ctx, name, audio, steps=None):
    """the restatement driven by a second product state: full() on its windows with its prompts, in order"""
    st = ctx.create_state()

    def run(pcm, prompt):
        st.full(GG.full_params(lib, name, prompt), pcm)
        return segs_of(st)

    ref = StreamRef(*GG.CONFIGS[name][0])
    n = len(audio) if steps is None else steps * ref.n_samples_step
    try:
        return drive(ref, audio[:n], run)
    finally:
        st.free()


@pytest.fixture(scope="module")
def sessions(wrs, amd_lib, ctx, audio):
    """each configuration once: the 12 s in 100 ms packets"""
    out = {}
    for name in (A, B):
        s = wrs.WhisperStream(ctx, **stream_kw(name))
        out[name] = run_session(wrs, amd_lib, s, name, audio, 1600)
        s.close()
    return out


# ---- 1. the session against the restatement ----
@pytest.mark.parametrize("name", [A, B])
def test_session_is_the_restatement(wrs, amd_lib, ctx, audio, sessions, name):
    want = restated(wrs, amd_lib, ctx, name, audio)
    z = StreamRef(*GG.CONFIGS[name][0])
    assert len(want) == {A: 12, B: 4}[name] and z.n_new_line == {A: 3, B: 1}[name]
    check_against(sessions[name], want, z)
    assert any(r["committed"] and r["prompt"] != want[k + 1]["prompt"] for k, r in enumerate(want[:-1])), "no commit changed the prompt"


# ---- 2. the reference engine's goldens ----
@pytest.mark.parametrize("name", [A, B])
def test_session_equals_the_reference_engine(golden, sessions, name):
    g = golden["configs"][name]
    assert g["step_length_keep"] == list(GG.CONFIGS[name][0]) and GG.ok(g["met"])
    want = g["windows"]
    assert len(want) == len(sessions[name]) == {A: 12, B: 4}[name]
    for k, (w, r) in enumerate(zip(sessions[name], want)):
        assert len(w["pcm"]) == r["n_samples"] and w["info"]["take"] == r["take"], k
        assert w["prompt"] == r["prompt"] and w["info"]["committed"] == (1 if r["committed"] else 0), k
        assert w["segs"] == r["segs"], ("the reference engine's segments", k)


# ---- 3. packet size and input format do not matter ----
def recording_44k(seed, seconds):
    """a 44.1 kHz stereo I16 recording: wsynth audio stretched by linear interpolation, the channels a little apart"""
    x = wsynth.synth_audio(16000 * seconds, seed).astype(np.float64)
    n = 44100 * seconds
    y = np.interp(np.arange(n) * (16000.0 / 44100.0), np.arange(len(x)), x)
    lr = np.stack([y * 0.9, y * 0.8 + 0.01], axis=1)
    return np.clip(np.round(lr * 32767.0), -32768, 32767).astype(np.int16).reshape(-1)


def test_packets_and_format_do_not_matter(wrs, amd_lib, ctx):
    seconds, rate = 5, 44100
    rec = recording_44k(3, seconds)
    n_frames = rate * seconds
    rng = np.random.default_rng(5)
    cuts = np.sort(rng.choice(np.arange(1, n_frames), 97, replace=False))
    ways = dict(p10ms=[441] * (n_frames // 441), p1s=[rate] * seconds, irregular=[int(v) for v in np.diff(np.concatenate([[0], cuts, [n_frames]]))])
    st = ctx.create_state()
    st.audio_to_pcm(rec, 2, rate, I16)
    whole = st.audio_copy()
    st.free()
    assert len(whole) == 16000 * seconds
    runs = {}
    for way, sizes in ways.items():
        assert sum(sizes) == n_frames
        s = wrs.WhisperStream(ctx, **stream_kw(A, sample_rate=rate, channels=2, format=I16))
        runs[way] = run_session(wrs, amd_lib, s, A, rec, sizes, channels=2, flush=True)
        s.close()
    first = runs["p10ms"]
    assert len(first) == seconds                    # the flush releases the filter's tail: the fifth second is complete only then
    for way, r in runs.items():
        assert len(r) == len(first), way
        for k, (a, b) in enumerate(zip(r, first)):
            assert np.array_equal(bits(a["pcm"]), bits(b["pcm"])) and a["segs"] == b["segs"] and a["prompt"] == b["prompt"], (way, k)
        axis = np.concatenate([w["pcm"][-16000:] for w in r])          # every window's new samples
        assert np.array_equal(bits(axis), bits(whole)), way
    assert len({json.dumps(w["segs"]) for w in first}) > 1


# ---- 4. eight sessions per tick ----
def feed_plan(tick, i):
    """samples session i holds after `tick`: sessions 6 and 7 are fed half a step late"""
    return tick * 16000 - (8000 if i >= 6 else 0)


def solo_runs(wrs, lib, c, audios, ticks):
    fp = GG.full_params(lib, A, None)
    out = []
    for i, a in enumerate(audios):
        s = wrs.WhisperStream(c, **stream_kw(A))
        rows, at = [], 0
        for tick in range(1, ticks + 1):
            assert s.feed(a[at:feed_plan(tick, i)]) >= 0
            at = feed_plan(tick, i)
            r = s.step(fp)
            assert r in (0, 1)
            rows.append(dict(segs=segs_of(s.state), pcm=s.window(), prompt=s.prompt()) if r else None)
        out.append(rows)
        s.close()
    return out


def many_runs(wrs, lib, c, audios, ticks):
    fp = GG.full_params(lib, A, None)
    ss = [wrs.WhisperStream(c, **stream_kw(A)) for _ in audios]
    out, at, stats = [[] for _ in audios], [0] * len(audios), []
    for tick in range(1, ticks + 1):
        due = 0
        for i, (s, a) in enumerate(zip(ss, audios)):
            d = s.feed(a[at[i]:feed_plan(tick, i)])
            assert d in (0, 1)
            due += d
            at[i] = feed_plan(tick, i)
        assert wrs.stream_step_many(ss, fp) == due
        stats.append((due,) + wrs.batch_stats(c))
        for i, s in enumerate(ss):
            ran = s.info()["windows"] == len([r for r in out[i] if r]) + 1
            out[i].append(dict(segs=segs_of(s.state), pcm=s.window(), prompt=s.prompt()) if ran else None)
    for s in ss:
        s.close()
    return out, stats


@pytest.fixture(scope="module")
def eight(wrs, amd_lib, ctx):
    audios = [wsynth.synth_audio(16000 * 6, seed) for seed in range(8)]
    return audios, solo_runs(wrs, amd_lib, ctx, audios, 6)


def same_rows(got, want):
    for i, (g, w) in enumerate(zip(got, want)):
        assert [r is None for r in g] == [r is None for r in w[:len(g)]], i
        for k, (a, b) in enumerate(zip(g, w)):
            if a:
                assert a["segs"] == b["segs"] and a["prompt"] == b["prompt"] and np.array_equal(bits(a["pcm"]), bits(b["pcm"])), (i, k)


def test_eight_sessions_per_tick(wrs, amd_lib, ctx, eight):
    audios, solo = eight
    got, stats = many_runs(wrs, amd_lib, ctx, audios, 6)
    assert [s[0] for s in stats] == [6, 8, 8, 8, 8, 8]
    same_rows(got, solo)
    assert sum(1 for rows in solo for r in rows if r) == 6 * 6 + 2 * 5
    assert len({json.dumps(r["segs"]) for rows in solo for r in rows if r}) > 8
    for due, passes, rows in stats:
        assert passes > 0 and rows > passes, "no lock-step passes served several rows: %r" % ((due, passes, rows),)


def test_eight_sessions_on_the_chaos_build(wrs, eight):
    audios, solo = eight
    path = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(path)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    c = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(lib, flash_attn=False), lib=lib)
    try:
        got, stats = many_runs(wrs, lib, c, audios, 2)
        assert [s[0] for s in stats] == [6, 8]
        same_rows(got, solo)
    finally:
        c.free()


# ---- 5. a quantised model ----
def test_q5_0_session(wrs, amd_lib, audio):
    c = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s128", "q5_0"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    try:
        s = wrs.WhisperStream(c, **stream_kw(A))
        got = run_session(wrs, amd_lib, s, A, audio[:48000], 1600)
        s.close()
        check_against(got, restated(wrs, amd_lib, c, A, audio, steps=3), StreamRef(*GG.CONFIGS[A][0]))
        assert len(got) == 3 and any(w["segs"] for w in got)
    finally:
        c.free()


# ---- 6. edges ----
def test_flush_gives_a_short_last_window(wrs, amd_lib, ctx, audio):
    s = wrs.WhisperStream(ctx, **stream_kw(A))
    got = run_session(wrs, amd_lib, s, A, audio[:36800], [1600] * 23, flush=True)
    assert [len(w["pcm"]) for w in got] == [16000, 32000, 36800] and got[2]["info"]["take"] == 32000
    assert np.array_equal(bits(got[2]["pcm"]), bits(audio[:36800]))
    assert s.info()["pending"] == 0 and s.feed(audio[:160]) == wrs.STREAM_ENDED
    st = ctx.create_state()
    st.full(GG.full_params(amd_lib, A, None), audio[:36800])
    assert got[2]["segs"] == segs_of(st) and got[2]["prompt"] == []
    st.free()
    s.close()


def test_flush_with_less_than_100_ms_left(wrs, amd_lib, ctx, audio):
    s = wrs.WhisperStream(ctx, step_ms=1000, length_ms=1000, keep_ms=0)      # nothing is kept: the last window is the 50 ms alone
    fp = GG.full_params(amd_lib, A, None)
    assert s.feed(audio[:16800]) == 1 and s.step(fp) == 1 and len(segs_of(s.state)) > 0
    assert s.info()["committed"] == 1 and s.flush() == 1 and s.step(fp) == 1
    i = s.info()
    assert (i["windows"], i["start"], i["length"], i["take"], i["pending"]) == (2, 16000, 800, 0, 0)
    assert segs_of(s.state) == [] and np.array_equal(bits(s.window()), bits(audio[16000:16800]))
    s.close()


def test_reset(wrs, amd_lib, ctx, audio, sessions):
    s = wrs.WhisperStream(ctx, **stream_kw(A))
    run_session(wrs, amd_lib, s, A, audio[:16000 * 4 + 700], [4900] * 13 + [1000])
    assert s.info()["windows"] == 4 and s.prompt() != []
    s.reset()
    i = s.info()
    assert (i["windows"], i["pending"], i["dropped"], i["length"]) == (0, 0, 0, 0)
    got = run_session(wrs, amd_lib, s, A, audio[:16000], 1600)
    assert len(got) == 1 and got[0]["segs"] == sessions[A][0]["segs"] and got[0]["prompt"] == [] and np.array_equal(bits(got[0]["pcm"]), bits(audio[:16000]))
    s.close()


def test_full_leaves_the_ring_as_it_was(wrs, amd_lib, ctx, audio):
    s = wrs.WhisperStream(ctx, **stream_kw(A, backlog_ms=2000))              # holds 2 n_step + 1 = 32 001 unconsumed samples
    fp = GG.full_params(amd_lib, A, None)
    assert s.feed(audio[:32000]) == 2 and s.feed(audio[32000:32001]) == 2
    before = s.info()
    assert s.feed(audio[32001:33601]) == wrs.STREAM_FULL
    assert s.info() == before and before["pending"] == 2 and before["dropped"] == 0
    assert s.step(fp) == 1 and np.array_equal(bits(s.window()), bits(audio[:16000]))
    assert s.feed(audio[32001:33601]) == 1                                   # room again; the refused packet was not half taken
    assert s.step(fp) == 1 and np.array_equal(bits(s.window()), bits(audio[:32000]))
    assert s.feed(audio[33601:48000]) == 1 and s.step(fp) == 1 and np.array_equal(bits(s.window()), bits(audio[:48000]))
    s.close()


def test_drop_late(wrs, amd_lib, ctx, audio):
    s = wrs.WhisperStream(ctx, **stream_kw(A, drop_late=1, backlog_ms=3000))
    fp = GG.full_params(amd_lib, A, None)
    assert s.feed(audio[:16000]) == 1 and s.step(fp) == 1
    assert s.feed(audio[16000:48000]) == 2 and s.step(fp) == 1               # 2 n_step pending: nothing is dropped
    assert np.array_equal(bits(s.window()), bits(audio[:32000])) and s.info()["dropped"] == 0
    assert s.feed(audio[48000:64001]) == 2                                   # 2 n_step + 1 pending
    assert s.step(fp) == 0
    i = s.info()
    assert (i["windows"], i["dropped"], i["pending"]) == (2, 32001, 0)
    assert s.feed(audio[64001:80001]) == 1 and s.step(fp) == 1
    i = s.info()
    assert (i["windows"], i["start"], i["length"], i["take"], i["dropped"]) == (3, 0, 48000, 32000, 32001)
    assert np.array_equal(bits(s.window()), bits(np.concatenate([audio[:32000], audio[64001:80001]])))
    st = ctx.create_state()
    st.full(GG.full_params(amd_lib, A, s.prompt()), s.window())
    assert segs_of(s.state) == segs_of(st)
    st.free()
    s.close()


def child_main():
    """one session at 16 kHz F32 and one at 44.1 kHz stereo I16, three windows each: digests of windows and segments, and the feed counts"""
    import whisper_rs as W
    lib = W.load_library()
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    c = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(lib, flash_attn=False), lib=lib)
    out = {}
    for tag, kw, data, packet, ch in (("f32_16k", {}, wsynth.synth_audio(48000, 0), 1600, 1),
                                     ("i16_44k", dict(sample_rate=44100, channels=2, format=I16), recording_44k(3, 3), 4410, 2)):
        s = W.WhisperStream(c, **stream_kw(A, **kw))
        rows = run_session(W, lib, s, A, data, packet, channels=ch, flush=True)
        h = hashlib.sha256()
        for w in rows:
            h.update(w["pcm"].tobytes()); h.update(json.dumps([w["segs"], w["prompt"]]).encode())
        i = s.info()
        out[tag] = dict(digest=h.hexdigest(), windows=len(rows), feeds_device=i["feeds_device"], feeds_host=i["feeds_host"])
        s.close()
    c.free()
    print("RESULT " + json.dumps(out))


def test_host_path_gives_the_same_digests():
    def child(host):
        env = dict(os.environ)
        env.pop("WHISPER_AMD_STREAM_HOST", None)
        if host:
            env["WHISPER_AMD_STREAM_HOST"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    dev, host = child(False), child(True)
    for tag in ("f32_16k", "i16_44k"):
        assert dev[tag]["windows"] == host[tag]["windows"] == 3 and dev[tag]["digest"] == host[tag]["digest"], tag
        assert dev[tag]["feeds_host"] == 0 and dev[tag]["feeds_device"] > 0 and host[tag]["feeds_device"] == 0 and host[tag]["feeds_host"] > 0, (dev[tag], host[tag])


def test_refusals(wrs, amd_lib, ctx, audio):
    def refused(**kw):
        with pytest.raises(wrs.WhisperError):
            wrs.WhisperStream(ctx, **kw)
    refused(sample_rate=16001); refused(sample_rate=7999); refused(channels=3); refused(channels=0); refused(format=2)
    refused(step_ms=0); refused(step_ms=-1000); refused(step_ms=1000, length_ms=29900, keep_ms=200)
    p = wrs.stream_params(amd_lib)
    assert not amd_lib.whisper_amd_stream_open(None, C.byref(p)) and not amd_lib.whisper_amd_stream_open(ctx.ptr, None)
    fp = GG.full_params(amd_lib, A, None)
    lib = amd_lib
    assert lib.whisper_amd_stream_feed(None, None, 0) == wrs.STREAM_BAD_ARGS and lib.whisper_amd_stream_flush(None) == wrs.STREAM_BAD_ARGS
    assert lib.whisper_amd_stream_step(None, C.byref(fp.c)) == wrs.STREAM_BAD_ARGS and lib.whisper_amd_stream_pending(None) == wrs.STREAM_BAD_ARGS
    assert lib.whisper_amd_stream_step_many(None, 1, C.byref(fp.c)) == wrs.STREAM_BAD_ARGS and lib.whisper_amd_stream_info(None, None) == wrs.STREAM_BAD_ARGS
    assert lib.whisper_amd_stream_window_copy(None, None, 0) == wrs.STREAM_BAD_ARGS and lib.whisper_amd_stream_prompt_copy(None, None, 0) == wrs.STREAM_BAD_ARGS
    assert lib.whisper_amd_stream_state(None) is None
    lib.whisper_amd_stream_close(None); lib.whisper_amd_stream_reset(None); lib.whisper_amd_stream_default_params(None)
    s = wrs.WhisperStream(ctx, **stream_kw(A))
    before = s.info()
    assert lib.whisper_amd_stream_feed(s.ptr, None, 5) == wrs.STREAM_BAD_ARGS and lib.whisper_amd_stream_feed(s.ptr, C.c_void_p(audio.ctypes.data), -1) == wrs.STREAM_BAD_ARGS
    assert lib.whisper_amd_stream_step(s.ptr, None) == wrs.STREAM_BAD_ARGS and s.info() == before
    many = (C.c_void_p * 65)(*([s.ptr] * 65))
    assert lib.whisper_amd_stream_step_many(many, 65, C.byref(fp.c)) == wrs.STREAM_MIXED
    assert lib.whisper_amd_stream_step_many(many, 2, C.byref(fp.c)) == wrs.STREAM_BAD_ARGS          # one session twice
    assert lib.whisper_amd_stream_step_many(many, 0, C.byref(fp.c)) == wrs.STREAM_BAD_ARGS
    other = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=True), lib=amd_lib)
    try:
        t = wrs.WhisperStream(other, **stream_kw(A))                         # a flash_attn context is served
        assert s.feed(audio[:16000]) == 1 and t.feed(audio[:16000]) == 1
        assert wrs.stream_step_many([s, t], fp) == wrs.STREAM_MIXED
        assert s.info()["pending"] == 1 and t.info()["pending"] == 1 and s.info()["windows"] == 0
        assert t.step(fp) == 1 and np.array_equal(bits(t.window()), bits(audio[:16000])) and t.info()["windows"] == 1
        assert s.step(fp) == 1
        t.close()
    finally:
        other.free()
    assert s.flush() == 0 and s.feed(audio[:1600]) == wrs.STREAM_ENDED
    s.close()


if __name__ == "__main__" and "--child" in sys.argv:
    child_main()

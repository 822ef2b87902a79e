"""Live sessions that cut at pauses, end to end (whisper_amd_stream_open_vad): model s128, the synthetic VAD model of
tools/wsynth_vad.py, the recording of tools/gen_golden_stream_vad.py.

The yardstick is stated offline: the session's probabilities are whisper_vad_detect_speech on whisper_amd_audio_to_pcm of everything fed, its
utterances the ranges of whisper_vad_segments_from_probs on them, each result whisper_full_with_state of a second state on those samples and
that prompt - and, for the 16 kHz recording, what the REFERENCE engine recorded in tests/golden/stream_vad.json (P, S, ids, text, p, plog).
Packet size, input rate and format, the number of sessions polled and stepped together, the host ring and the stalls of the chaos build must
not change a result."""
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
import wsynth_vad as V
import gen_golden_stream_vad as GG
import stream_vad_ref as R

pytestmark = pytest.mark.gpu

I16, F32 = 0, 1
T = GG.N_SAMPLES


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def segs_of(state):
    return [dict(text=s["text"].decode("latin1"), ids=s["ids"], p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]])
            for s in state.segments()]


def record(s):
    u = s.utterance_info()
    return dict(pcm=s.window(), prompt=s.prompt(), segs=segs_of(s.state), seg=(u["start_cs"], u["end_cs"]), start=u["start"], length=u["length"], split=u["split"])


def run_session(lib, s, name, audio, packets, channels=1, flush=True):
    """feed `audio` (frames x channels, interleaved) in `packets` (frame counts); step whenever an utterance is due.  Returns the utterances and
    how many of them came before the flush."""
    fp = GG.full_params(lib, name, None)
    out = []

    def drain():
        while s.pending() > 0:
            assert s.step(fp) == 1
            out.append(record(s))
            assert s.utterance_info()["utterances"] == len(out)

    at = 0
    for n in packets:
        due = s.feed(audio[at * channels:(at + n) * channels])
        assert due >= 0 and due == s.pending(), due
        at += n
        drain()
    early = len(out)
    if flush:
        assert s.flush() == s.pending()
        drain()
    assert s.step(fp) == 0
    return out, early


def packets_of(n_frames, rate):
    rng = np.random.default_rng(11)
    cuts = np.sort(rng.choice(np.arange(1, n_frames), 83, replace=False))
    cut = lambda p: [p] * (n_frames // p) + ([n_frames % p] if n_frames % p else [])
    return dict(p10ms=cut(rate // 100), p100ms=cut(rate // 10), p1s=cut(rate), irregular=[int(v) for v in np.diff(np.concatenate([[0], cuts, [n_frames]]))])


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "stream_vad.json")))


@pytest.fixture(scope="module")
def x(golden):
    a = GG.recording()
    assert len(a) == golden["n_samples"] == T and golden["vad"] == GG.VAD and GG.ok(golden["met"])
    return a


@pytest.fixture(scope="module")
def ctx(wrs, amd_lib):
    c = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    yield c
    c.free()


@pytest.fixture(scope="module")
def vctx(wrs, amd_lib):
    v = wrs.WhisperVadContext.new(V.model_path(), lib=amd_lib)
    yield v
    v.free()


def offline(wrs, lib, vctx, pcm):
    """the yardstick on a whole 16 kHz recording: probabilities, segments, utterance ranges"""
    P = vctx.detect_speech(pcm)
    S = [(int(a), int(b)) for a, b in vctx.segments_from_probs(GG.vad_params(lib))]
    assert R.segments(P, GG.VAD) == S and R.capped(P, GG.VAD, GG.CAP_MS)[1] == 0
    return P, S, [R.utterance_range(s, len(pcm)) for s in S]


def check_session(got, early, probs, pcm, P, S, ranges):
    assert np.array_equal(bits(probs), bits(P)), "probabilities"
    assert [u["seg"] for u in got] == S and [(u["start"], u["length"]) for u in got] == ranges and all(u["split"] == 0 for u in got)
    for k, u in enumerate(got):
        a, n = ranges[k]
        assert np.array_equal(bits(u["pcm"]), bits(pcm[a:a + n])), ("utterance PCM", k)
    assert early == len(S) - 1 and ranges[-1][0] + ranges[-1][1] == len(pcm), "speech is running at the end: the last utterance comes with the flush"


# ---- 1. probabilities and utterances, however the input is cut ----
@pytest.mark.parametrize("way", ["p10ms", "p100ms", "p1s", "irregular"])
def test_16k_f32_mono(wrs, amd_lib, ctx, vctx, golden, x, way):
    P, S, ranges = offline(wrs, amd_lib, vctx, x)
    assert [int(b) for b in bits(P)] == golden["P"] and [list(s) for s in S] == golden["S"], "the product's whole-recording VAD against the reference's"
    s = wrs.WhisperVadStream(ctx, vctx)
    got, early = run_session(amd_lib, s, "greedy", x, packets_of(T, 16000)[way])
    check_session(got, early, s.probs(), x, P, S, ranges)
    i, u = s.info(), s.utterance_info()
    assert u["windows"] == len(P) == -(-T // 512) and i["feeds_host"] == 0 and i["feeds_device"] > 0 and i["windows"] == len(S)
    assert u["front_launches"] <= len(packets_of(T, 16000)[way]) + 1
    s.close()
    want = golden["configs"]["greedy"]["carry0"]
    assert [u["segs"] for u in got] == [w["segs"] for w in want] and all(u["prompt"] == [] for u in got)


def recording_44k(x):
    """the recording as 44.1 kHz stereo I16: stretched by linear interpolation, the channels a little apart"""
    n = 44100 * 13
    y = np.interp(np.arange(n) * (16000.0 / 44100.0), np.arange(len(x)), x.astype(np.float64))
    lr = np.stack([y * 0.9, y * 0.8 + 0.01], axis=1)
    return np.clip(np.round(lr * 32767.0), -32768, 32767).astype(np.int16).reshape(-1)


@pytest.fixture(scope="module")
def rec44(wrs, amd_lib, ctx, vctx, x):
    rec = recording_44k(x)
    st = ctx.create_state()
    st.audio_to_pcm(rec, 2, 44100, I16)
    whole = st.audio_copy()
    st.free()
    assert len(whole) == 16000 * 13
    return (rec, whole) + offline(wrs, amd_lib, vctx, whole)


@pytest.mark.parametrize("way", ["p10ms", "p100ms", "p1s", "irregular"])
def test_44k_i16_stereo(wrs, amd_lib, ctx, vctx, rec44, way):
    rec, whole, P, S, ranges = rec44
    assert len(S) >= 4
    s = wrs.WhisperVadStream(ctx, vctx, sample_rate=44100, channels=2, format=I16)
    got, early = run_session(amd_lib, s, "greedy", rec, packets_of(44100 * 13, 44100)[way], channels=2)
    check_session(got, early, s.probs(), whole, P, S, ranges)
    s.close()
    st = ctx.create_state()
    for k, u in enumerate(got):
        st.full(GG.full_params(amd_lib, "greedy", None), u["pcm"])
        assert u["segs"] == segs_of(st), k
    st.free()


# ---- 2. every result: a second state on those samples and that prompt, and the reference engine's record ----
@pytest.mark.parametrize("name", ["greedy", "beam3"])
@pytest.mark.parametrize("carry", [0, 1])
def test_results(wrs, amd_lib, ctx, vctx, golden, x, name, carry):
    s = wrs.WhisperVadStream(ctx, vctx, carry_prompt=carry)
    got, _ = run_session(amd_lib, s, name, x, packets_of(T, 16000)["p100ms"])
    s.close()
    want = golden["configs"][name]["carry%d" % carry]
    assert len(got) == len(want) >= 4
    st = ctx.create_state()
    for k, (u, w) in enumerate(zip(got, want)):
        assert (u["start"], u["length"], u["prompt"]) == (w["start"], w["n_samples"], w["prompt"]), k
        assert u["segs"] == w["segs"], ("the reference engine's segments", k)
        st.full(GG.full_params(amd_lib, name, u["prompt"]), x[u["start"]:u["start"] + u["length"]])
        assert u["segs"] == segs_of(st), ("a second state", k)
    st.free()
    if carry:
        assert any(u["prompt"] for u in got) and got[0]["prompt"] == []
        assert [u["segs"] for u in got] != [w["segs"] for w in golden["configs"][name]["carry0"]], "the prompt changed nothing"


# ---- 3. eight sessions: one front-end launch per poll, one gather per step_many ----
def audios_of(x):
    """eight recordings: the recording behind 0 .. 7 x 1700 samples of faint noise (the utterances lie elsewhere in the windows)"""
    rng = np.random.default_rng(5)
    return [np.concatenate([(0.002 * rng.standard_normal(1700 * i)).astype(np.float32), x])[:T] for i in range(8)]


def solo(wrs, lib, c, v, audios):
    out = []
    for a in audios:
        s = wrs.WhisperVadStream(c, v)
        got, _ = run_session(lib, s, "greedy", a, packets_of(T, 16000)["p100ms"])
        out.append((got, s.probs()))
        s.close()
    return out


def many(wrs, lib, c, v, audios, tick=3200):
    fp = GG.full_params(lib, "greedy", None)
    ss = [wrs.WhisperVadStream(c, v, vad_on_feed=0) for _ in audios]
    out, polls = [[] for _ in audios], 0

    def poll_and_step():
        nonlocal polls
        before = [s.utterance_info()["windows"] for s in ss]
        due = wrs.stream_vad_poll_many(ss)
        assert due == sum(s.pending() for s in ss) and wrs.stream_vad_poll_many(ss) == due          # a second poll has nothing to do
        polls += 1 if any(s.utterance_info()["windows"] != b for s, b in zip(ss, before)) else 0
        while due > 0:
            done = [s.utterance_info()["utterances"] for s in ss]
            ran = wrs.stream_step_many(ss, fp)
            assert 0 < ran <= due
            for i, s in enumerate(ss):
                if s.utterance_info()["utterances"] != done[i]:
                    out[i].append(record(s))
            due -= ran

    for at in range(0, T, tick):
        for s, a in zip(ss, audios):
            assert s.feed(a[at:at + tick]) == s.pending()               # vad_on_feed = 0: a feed makes nothing due
        poll_and_step()
    for s in ss:
        s.flush()
    poll_and_step()
    probs = [s.probs() for s in ss]
    launches = [s.utterance_info()["front_launches"] for s in ss]
    for s in ss:
        s.close()
    return out, probs, launches, polls


def same_runs(got, probs, want):
    for i, (w, p) in enumerate(want):
        assert np.array_equal(bits(probs[i]), bits(p)), i
        assert len(got[i]) == len(w) >= 4, i
        for k, (a, b) in enumerate(zip(got[i], w)):
            assert a["segs"] == b["segs"] and a["seg"] == b["seg"] and a["prompt"] == b["prompt"] and np.array_equal(bits(a["pcm"]), bits(b["pcm"])), (i, k)


@pytest.fixture(scope="module")
def eight(wrs, amd_lib, ctx, vctx, x):
    audios = audios_of(x)
    return audios, solo(wrs, amd_lib, ctx, vctx, audios)


def test_eight_sessions_per_tick(wrs, amd_lib, ctx, vctx, eight):
    audios, want = eight
    got, probs, launches, polls = many(wrs, amd_lib, ctx, vctx, audios)
    same_runs(got, probs, want)
    assert polls >= T // 3200 and launches == [polls] * 8, "one front-end launch per poll for the whole group"
    assert len({json.dumps(u["segs"]) for g in got for u in g}) > 8


def test_eight_sessions_on_the_chaos_build(wrs, eight):
    audios, want = eight
    path = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(path)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    c = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(lib, flash_attn=False), lib=lib)
    v = wrs.WhisperVadContext.new(V.model_path(), lib=lib)
    try:
        got, probs, launches, polls = many(wrs, lib, c, v, audios)
        same_runs(got, probs, want)
    finally:
        v.free()
        c.free()


# ---- 4. edges ----
def test_reset(wrs, amd_lib, ctx, vctx, x, golden):
    s = wrs.WhisperVadStream(ctx, vctx, carry_prompt=1)
    got, _ = run_session(amd_lib, s, "greedy", x[:16000 * 7], [1600] * 70, flush=False)
    assert len(got) == 2 and s.utterance_info()["windows"] == 16000 * 7 // 512
    s.reset()
    u, i = s.utterance_info(), s.info()
    assert (u["utterances"], u["windows"], u["front_launches"], u["length"], i["pending"], len(s.probs())) == (0, 0, 0, 0, 0, 0)
    got, _ = run_session(amd_lib, s, "greedy", x, packets_of(T, 16000)["p100ms"])
    want = golden["configs"]["greedy"]["carry1"]
    assert [u["segs"] for u in got] == [w["segs"] for w in want] and [u["prompt"] for u in got] == [w["prompt"] for w in want]
    assert [int(b) for b in bits(s.probs())] == golden["P"]
    s.close()


def test_full_leaves_everything_as_it_was(wrs, amd_lib, ctx, vctx, x, golden):
    """a ring of 2 s + 40 192 samples; nothing is stepped, so the first utterance (from sample 13 280 on) must stay: 53 packets of 100 ms fit"""
    vad = dict(max_speech_duration_s=2.0)
    s = wrs.WhisperVadStream(ctx, vctx, vad=vad, max_utterance_ms=2000, backlog_ms=0)
    first = R.utterance_range(golden["S"][0], T)
    assert first[0] == 13280
    ring = 32000 + 32000 + 8192
    fits = [k for k in range(200) if 1600 * (k + 1) - first[0] <= ring][-1] + 1
    assert fits == 53
    for k in range(fits):
        assert s.feed(x[1600 * k:1600 * (k + 1)]) >= 0, k
    before = (s.info(), s.utterance_info(), s.probs().tobytes())
    assert before[0]["pending"] >= 1
    assert s.feed(x[1600 * fits:1600 * (fits + 1)]) == wrs.STREAM_FULL
    assert (s.info(), s.utterance_info(), s.probs().tobytes()) == before
    fp = GG.full_params(amd_lib, "greedy", None)
    assert s.step(fp) == 1 and np.array_equal(bits(s.window()), bits(x[first[0]:first[0] + first[1]]))
    assert s.feed(x[1600 * fits:1600 * (fits + 1)]) >= 0                 # room again; the refused packet was not half taken
    segs = [s.utterance_info()["start_cs"]]
    for at in list(range(1600 * (fits + 1), T, 1600)) + [None]:            # the rest, then the flush: everything still comes out, in order
        assert (s.feed(x[at:at + 1600]) if at is not None else s.flush()) >= 0
        while s.pending() > 0:
            assert s.step(fp) == 1
            segs.append(s.utterance_info()["start_cs"])
    assert segs == [a for a, _ in golden["S"]] and [int(b) for b in bits(s.probs())] == golden["P"]
    s.close()


def long_speech():
    """7 s with one burst of 5 s"""
    n = 16000 * 7
    rng = np.random.default_rng(9)
    t = np.arange(n, dtype=np.float64) / 16000.0
    env = ((t >= 0.5) & (t < 5.5)).astype(np.float64)
    a = env * (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * (500.0 + 100.0 * t) * t)) + 0.002 * rng.standard_normal(n)
    return a.astype(np.float32)


def test_split_at_the_cap(wrs, amd_lib, ctx, vctx):
    a = long_speech()
    vad = dict(GG.VAD, max_speech_duration_s=2.0)
    P = vctx.detect_speech(a)
    want, splits = R.capped(P, vad, 2000)
    assert splits >= 1 and len(want) >= 2 and len(R.segments(P, vad)) < len(want), "the offline list re-joins what max_speech split"
    s = wrs.WhisperVadStream(ctx, vctx, vad=dict(max_speech_duration_s=2.0), max_utterance_ms=2000)
    got, _ = run_session(amd_lib, s, "greedy", a, [1600] * 70)
    assert np.array_equal(bits(s.probs()), bits(P))
    s.close()
    assert [u["seg"] + (u["split"],) for u in got] == [(a0, b0, 1 if sp else 0) for a0, b0, sp in want]
    for u, w in zip(got, want):
        r = R.utterance_range(w[:2], len(a))
        assert (u["start"], u["length"]) == r and 0 < r[1] <= 32000 and np.array_equal(bits(u["pcm"]), bits(a[r[0]:r[0] + r[1]]))


def test_refusals(wrs, amd_lib, ctx, vctx, x):
    lib = amd_lib

    def refused(vad=None, **kw):
        with pytest.raises(wrs.WhisperError):
            wrs.WhisperVadStream(ctx, vctx, vad=vad, **kw)
    refused(sample_rate=16001); refused(sample_rate=7999); refused(channels=3); refused(channels=0); refused(format=2)
    refused(vad=dict(speech_pad_ms=101)); refused(vad=dict(speech_pad_ms=-1)); refused(max_utterance_ms=0); refused(max_utterance_ms=30001)
    refused(vad=dict(max_speech_duration_s=30.5)); refused(vad=dict(max_speech_duration_s=float(np.finfo(np.float32).max)))
    refused(vad=dict(max_speech_duration_s=10.0), max_utterance_ms=9999); refused(backlog_ms=-1)
    wrs.WhisperVadStream(ctx, vctx, vad=dict(max_speech_duration_s=10.0, speech_pad_ms=100), max_utterance_ms=10000).close()
    p = wrs.stream_vad_params(lib)
    assert not lib.whisper_amd_stream_open_vad(None, vctx.ptr, C.byref(p)) and not lib.whisper_amd_stream_open_vad(ctx.ptr, None, C.byref(p))
    assert not lib.whisper_amd_stream_open_vad(ctx.ptr, vctx.ptr, None)
    lib.whisper_amd_stream_vad_default_params(None)
    n_dev = __import__("torch").cuda.device_count()
    if n_dev > 1:
        other = wrs.WhisperVadContext.new(V.model_path(), lib=lib, gpu_device=1)
        assert not lib.whisper_amd_stream_open_vad(ctx.ptr, other.ptr, C.byref(p))
        other.free()
    assert lib.whisper_amd_stream_vad_poll_many(None, 1) == wrs.STREAM_BAD_ARGS and lib.whisper_amd_stream_utterance_info(None, None) == wrs.STREAM_BAD_ARGS
    assert lib.whisper_amd_stream_vad_probs_copy(None, None, 0) == wrs.STREAM_BAD_ARGS
    s, w = wrs.WhisperVadStream(ctx, vctx), wrs.WhisperStream(ctx, step_ms=1000, length_ms=4000, keep_ms=200)
    out = (C.c_int64 * 8)()
    assert lib.whisper_amd_stream_utterance_info(w.ptr, out) == wrs.STREAM_BAD_ARGS and lib.whisper_amd_stream_vad_probs_copy(w.ptr, None, 0) == wrs.STREAM_BAD_ARGS
    assert wrs.stream_vad_poll_many([s, w]) == wrs.STREAM_MIXED and wrs.stream_vad_poll_many([s, s]) == wrs.STREAM_BAD_ARGS
    assert lib.whisper_amd_stream_vad_poll_many((C.c_void_p * 65)(*([s.ptr] * 65)), 65) == wrs.STREAM_MIXED
    v2 = wrs.WhisperVadContext.new(V.model_path(), lib=lib)
    t = wrs.WhisperVadStream(ctx, v2)
    assert wrs.stream_vad_poll_many([s, t]) == wrs.STREAM_MIXED                  # two VAD contexts
    t.close(); v2.free()
    assert wrs.stream_vad_poll_many([s]) == 0 and s.flush() == 0 and s.feed(x[:1600]) == wrs.STREAM_ENDED
    with pytest.raises(wrs.WhisperError):
        wrs.WhisperStream(ctx, step_ms=0)                                        # step mode keeps refusing step_ms <= 0
    s.close(); w.close()


# ---- 5. the host ring, in a fresh process ----
def child_main():
    """the recording at 16 kHz F32 and at 44.1 kHz stereo I16: digests of probabilities, utterances and segments, and the feed counts"""
    import whisper_rs as W
    lib = W.load_library()
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    c = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(lib, flash_attn=False), lib=lib)
    v = W.WhisperVadContext.new(V.model_path(), lib=lib)
    a = GG.recording()
    out = {}
    for tag, kw, data, packet, ch in (("f32_16k", {}, a, packets_of(T, 16000)["irregular"], 1),
                                     ("i16_44k", dict(sample_rate=44100, channels=2, format=I16), recording_44k(a), packets_of(44100 * 13, 44100)["p100ms"], 2)):
        s = W.WhisperVadStream(c, v, **kw)
        rows, _ = run_session(lib, s, "greedy", data, packet, channels=ch)
        h = hashlib.sha256()
        h.update(s.probs().tobytes())
        for u in rows:
            h.update(u["pcm"].tobytes()); h.update(json.dumps([u["segs"], u["prompt"], u["seg"], u["start"]]).encode())
        i = s.info()
        out[tag] = dict(digest=h.hexdigest(), utterances=len(rows), feeds_device=i["feeds_device"], feeds_host=i["feeds_host"])
        s.close()
    v.free()
    c.free()
    print("RESULT " + json.dumps(out))


def test_host_ring_gives_the_same_digests():
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
        assert dev[tag]["utterances"] == host[tag]["utterances"] >= 4 and dev[tag]["digest"] == host[tag]["digest"], tag
        assert dev[tag]["feeds_host"] == 0 and dev[tag]["feeds_device"] > 0 and host[tag]["feeds_device"] == 0 and host[tag]["feeds_host"] > 0, (dev[tag], host[tag])


if __name__ == "__main__" and "--child" in sys.argv:
    child_main()

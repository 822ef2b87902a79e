"""The sample formats beyond int16 and F32 - U8, packed S24, S32, F64, G.711 mu-law and A-law - and the WAV header parser, through the C ABI
(model s128 where a model is needed).

Every comparison is bit for bit and rests on the equivalences csrc/wa_audio.h states: G.711 input gives what I16 input holding the expanded
samples gives, and U8 / S24 / S32 / F64 input what F32 input holding the per-sample v / S (F64: v) gives, at the same channel count and rate.
tests/test_audio_formats_math.py holds the host restatement to the same equivalences and to numpy arithmetic written out; the I16 and F32
kernels are held to the restatement by tests/test_audio_kernels_gpu.py."""
import ctypes as C
import hashlib
import json
import math
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT              # first: it puts tools/ and whisper-rust_amd/ on the path, also for the child process below

import channels_cases as K
import gen_golden_stream as GS
import gen_golden_stream_vad as GV
import wsynth
import wsynth_vad as V

pytestmark = pytest.mark.gpu

I16, F32, U8, S24, S32, F64, ULAW, ALAW = 0, 1, 3, 4, 5, 6, 7, 8
NEW = [U8, S24, S32, F64, ULAW, ALAW]
SCALE = {U8: 128.0, S24: 8388608.0, S32: 2147483648.0, ULAW: 32768.0, ALAW: 32768.0}
PACKETS = [1, 159, 160, 161, 4000]
STREAM = "greedy_1000_4000_200"


def plan_of(rate):
    g = math.gcd(rate, 16000)
    L, M = 16000 // g, rate // g
    return L, M, 0 if rate == 16000 else 64 * -(-max(L, M) // L)


def n_out_of(n_frames, rate):
    return -(-n_frames * 16000 // rate)


def frames_for(n_out, rate):
    """the shortest input that gives n_out samples (at least n_out below 16 kHz), as tests/test_audio_kernels_gpu.py chooses it"""
    return (n_out - 1) * rate // 16000 + 1


def lengths_of(rate, tile):
    K_ = plan_of(rate)[2] or 64
    around = [K_ // 2 - 1, K_, frames_for(3 * tile, rate) + 17, frames_for(tile - 1, rate) - 1, frames_for(tile - 1, rate), frames_for(tile, rate), frames_for(tile + 1, rate)]
    return [1, 2, 3, 15, 16, 17, 47, 48, 49] + around          # 47 .. 49: either side of a 48-byte group of S24 samples


def device_offsets(fmt):
    return (0, 4) if fmt == S32 else (0, 8) if fmt == F64 else (0, 1, 2, 3)


def make_input(wrs, rng, n, fmt):
    """n samples of a new format, the extremes first: (the array the entry reads, its values v as float32)"""
    def lead(x, ext):
        x[:min(n, len(ext))] = ext[:min(n, len(ext))]
        return x
    if fmt == U8:
        x = lead(rng.integers(0, 256, n).astype(np.uint8), np.array([0, 255, 255, 0, 128, 127], np.uint8))
        return x, (x.astype(np.int32) - 128).astype(np.float32)
    if fmt == S24:
        s = lead(rng.integers(-2 ** 23, 2 ** 23, n).astype(np.int32), np.array([2 ** 23 - 1, -2 ** 23, -(2 ** 23 - 1), 2 ** 23 - 1, -2 ** 23, -2 ** 23, 0, -1], np.int32))
        return wrs.pack_s24(s), s.astype(np.float32)
    if fmt == S32:
        s = lead(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
                 np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 31 - 65, 2 ** 31 - 64], np.int32))
        return s, s.astype(np.float32)
    if fmt == F64:
        x = lead(rng.uniform(-1.0, 1.0, n), np.array([1.0, -1.0, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e-40, -1e-40, 0.1, 2.0 ** -126 * (1 - 2.0 ** -25)]))
        return x, x.astype(np.float32)
    x = lead(rng.integers(0, 256, n).astype(np.uint8), np.array([0x00, 0x80, 0x7F, 0xFF, 0x55, 0xD5, 0x2A, 0xAA, 0x01], np.uint8))
    return x, (wrs.ulaw_to_linear(x) if fmt == ULAW else wrs.alaw_to_linear(x)).astype(np.float32)


def equivalent(x, v, fmt):
    """(format, array) of the input the I16 / F32 kernels serve with the same bits"""
    if fmt in (ULAW, ALAW):
        return I16, v.astype(np.int16)
    return F32, (v if fmt == F64 else v / np.float32(SCALE[fmt]))


def same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: %d of %d samples differ, first at %d: %r != %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


class DeviceBuffer:
    """device memory behind a 256-byte boundary; put(x, offset) copies a host array `offset` bytes behind that boundary"""
    def __init__(self, nbytes):
        self.hip = C.CDLL("libamdhip64.so")
        self.base, self.cap = C.c_void_p(), nbytes
        assert self.hip.hipMalloc(C.byref(self.base), C.c_size_t(nbytes + 512)) == 0
        self.start = (self.base.value + 255) // 256 * 256

    def put(self, x, offset=0):
        assert x.nbytes + offset <= self.cap
        assert self.hip.hipMemcpy(C.c_void_p(self.start + offset), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0
        return self.start + offset

    def free(self):
        self.hip.hipFree(self.base)


@pytest.fixture(scope="module")
def ctx(wrs, amd_lib):
    c = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    yield c
    c.free()


@pytest.fixture(scope="module")
def fctx(wrs, amd_lib):
    c = wrs.WhisperFullContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    yield c
    c.free()


@pytest.fixture(scope="module")
def vctx(wrs, amd_lib):
    v = wrs.WhisperVadContext.new(V.model_path(), lib=amd_lib)
    yield v
    v.free()


@pytest.fixture(scope="module")
def tile(amd_lib):
    return amd_lib.whisper_amd_audio_tile()


@pytest.fixture(scope="module")
def dev():
    d = DeviceBuffer(1 << 20)
    yield d
    d.free()


# ---- whisper_amd_audio_to_pcm ----
@pytest.mark.parametrize("fmt", NEW)
def test_to_pcm_is_the_equivalent_call(wrs, ctx, tile, dev, fmt):
    """every length, channel count and rate; a host pointer and device copies 0 .. 3 bytes (S32: 0, 4; F64: 0, 8) behind a 256-byte boundary"""
    rng = np.random.default_rng(100 + fmt)
    st, twin = ctx.create_state(), ctx.create_state()
    calls = 0
    for rate in (8000, 16000, 48000):
        for ch in (1, 2):
            for n in lengths_of(rate, tile):
                x, v = make_input(wrs, rng, n * ch, fmt)
                efmt, ex = equivalent(x, v, fmt)
                twin.audio_to_pcm(ex, ch, rate, efmt)
                want = twin.audio_copy()
                assert len(want) == n_out_of(n, rate) and np.all(np.isfinite(want))
                # the host pointer 1 byte into a buffer for the byte formats: a WAV image's samples lie anywhere
                hx = np.concatenate([np.zeros(1, np.uint8), x.view(np.uint8)])[1:] if fmt in (U8, S24, ULAW, ALAW) else x
                ptr, got_n = st.audio_to_pcm(hx, ch, rate, fmt)
                assert ptr and got_n == len(want)
                same(st.audio_copy(), want, "host pointer, fmt %d rate %d ch %d n %d" % (fmt, rate, ch, n))
                calls += 1
                for off in device_offsets(fmt):
                    ptr2, got_n = st.audio_to_pcm((dev.put(x, off), n), ch, rate, fmt)
                    assert ptr2 == ptr and got_n == len(want)
                    same(st.audio_copy(), want, "device pointer + %d, fmt %d rate %d ch %d n %d" % (off, fmt, rate, ch, n))
                    calls += 1
    assert st.audio_stats() == (calls, 0, 0)                    # the kernels served every call: nothing fell back to the host
    assert twin.audio_stats()[1:] == (0, 0)
    st.free()
    twin.free()


def test_f64_nan_and_inf_pass_through(wrs, ctx, dev):
    x = np.array([0.25, np.nan, -0.5, np.inf, 0.125, -np.inf, 1e300, -1e300] * 8, np.float64)
    with np.errstate(over="ignore"):
        e = x.astype(np.float32)
    st, twin = ctx.create_state(), ctx.create_state()
    for ch in (1, 2):
        for rate in (16000, 48000):
            twin.audio_to_pcm(e, ch, rate, F32)
            want = twin.audio_copy()
            st.audio_to_pcm((dev.put(x), len(x) // ch), ch, rate, F64)
            same(st.audio_copy(), want, "ch %d rate %d" % (ch, rate))
            assert np.isnan(want).any()
    assert st.audio_stats() == (4, 0, 0)
    st.free()
    twin.free()


HOST_CASES = [(ULAW, 1, 8000, 2500), (S24, 2, 44100, 3001), (S32, 1, 48000, 2999), (F64, 2, 16000, 1500)]      # one format of each width


def host_case_digests(wrs, ctx):
    out = {}
    st = ctx.create_state()
    for fmt, ch, rate, n in HOST_CASES:
        x, _ = make_input(wrs, np.random.default_rng(900 + fmt), n * ch, fmt)
        st.audio_to_pcm(x, ch, rate, fmt)
        out["%d" % fmt] = hashlib.sha256(st.audio_copy().tobytes()).hexdigest()
    out["stats"] = list(st.audio_stats())
    st.free()
    return out


def child_main():
    import whisper_rs as wrs
    lib = wrs.load_library(os.path.join(ROOT, "whisper-rust_amd", "libwhisper.so"))
    c = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(lib, flash_attn=False), lib=lib)
    out = host_case_digests(wrs, c)
    c.free()
    print("RESULT " + json.dumps(out))


def test_host_path_gives_the_same_bits(wrs, ctx):
    """WHISPER_AMD_AUDIO_HOST=1 in a fresh child process: the host restatement serves the calls and gives what the kernels give here"""
    env = dict(os.environ, WHISPER_AMD_AUDIO_HOST="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    host = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    here = host_case_digests(wrs, ctx)
    assert here["stats"] == [len(HOST_CASES), 0, 0] and host["stats"] == [0, len(HOST_CASES), 0]
    for fmt, _, _, _ in HOST_CASES:
        assert host["%d" % fmt] == here["%d" % fmt], fmt


# ---- whisper_amd_audio_split ----
@pytest.mark.parametrize("fmt", NEW)
def test_split_planes(wrs, ctx, dev, fmt):
    """each plane is whisper_amd_audio_to_pcm of that channel as a mono recording in the same format, and the plane of the equivalent input's split"""
    rng = np.random.default_rng(200 + fmt)
    st, twin, mono = ctx.create_state(), ctx.create_state(), ctx.create_state()
    b = wrs.PCM_SAMPLE_BYTES[fmt]
    for rate in (8000, 44100):
        tile = st.lib.whisper_amd_channels_tile()
        for n in (1, 17, 49, frames_for(tile, rate) - 1, frames_for(tile + 1, rate), frames_for(2 * tile, rate) + 5):
            x, v = make_input(wrs, rng, 2 * n, fmt)
            efmt, ex = equivalent(x, v, fmt)
            twin.audio_split(ex, rate, efmt)
            want = [twin.audio_split_copy(c) for c in (0, 1)]
            for c in (0, 1):
                plane = np.ascontiguousarray(x.view(np.uint8).reshape(n, 2, b)[:, c, :]).reshape(-1).view(x.dtype)
                mono.audio_to_pcm(plane, 1, rate, fmt)
                same(mono.audio_copy(), want[c], "the channel as a mono recording: fmt %d rate %d n %d channel %d" % (fmt, rate, n, c))
            _, got_n, _ = st.audio_split(x, rate, fmt)
            assert got_n == n_out_of(n, rate)
            for c in (0, 1):
                same(st.audio_split_copy(c), want[c], "host pointer: fmt %d rate %d n %d channel %d" % (fmt, rate, n, c))
            for off in device_offsets(fmt):
                st.audio_split((dev.put(x, off), n), rate, fmt)
                for c in (0, 1):
                    same(st.audio_split_copy(c), want[c], "device pointer + %d: fmt %d rate %d n %d channel %d" % (off, fmt, rate, n, c))
    assert mono.audio_stats()[1:] == (0, 0)
    for s in (st, twin, mono):
        s.free()


# ---- the live feed ----
def segs_of(state):
    return [dict(text=s["text"].decode("latin1"), ids=s["ids"], p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]])
            for s in state.segments()]


def run_pair(lib, a, b, fp, feeds):
    """two sessions fed in step - feeds: [(packet for a, packet for b)] -; after every feed and the flush both run the windows that are due.
    Returns the records of a after checking b's against them."""
    out = []

    def drain():
        assert a.pending() == b.pending()
        while a.pending() > 0:
            assert a.step(fp) == 1 and b.step(fp) == 1
            wa, wb = a.window(), b.window()
            same(wa, wb, "window %d" % len(out))
            ra, rb = segs_of(a.state), segs_of(b.state)
            assert ra == rb, ("segments of window %d" % len(out))
            out.append(dict(pcm=wa, segs=ra))

    for pa, pb in feeds:
        da, db = a.feed(pa), b.feed(pb)
        assert da >= 0 and da == db, (da, db)
        drain()
    assert a.flush() == b.flush()
    drain()
    ia, ib = a.info(), b.info()
    assert ia["feeds_host"] == 0 and ib["feeds_host"] == 0 and ia["feeds_device"] == ib["feeds_device"] > 0
    return out


def cuts_of(n_frames):
    at, k, cuts = 0, 0, []
    while at < n_frames:
        n = min(PACKETS[k % len(PACKETS)], n_frames - at)
        cuts.append((at, n))
        at, k = at + n, k + 1
    return cuts


def test_stream_ulaw_is_its_int16_twin(wrs, amd_lib, ctx):
    """8 kHz mono: mu-law packets of 1, 159, 160, 161 and 4000 frames in turn against the expanded int16 with the same packets"""
    pcm = wsynth.synth_audio(16000 * 4, 3)[::2]                                     # 4 s at 8 kHz
    codes = wrs.linear_to_ulaw(K.to_i16(pcm))
    lin = wrs.ulaw_to_linear(codes)
    kw = dict(step_ms=1000, length_ms=4000, keep_ms=200, sample_rate=8000, channels=1)
    a, b = wrs.WhisperStream(ctx, format=ULAW, **kw), wrs.WhisperStream(ctx, format=I16, **kw)
    out = run_pair(amd_lib, a, b, GS.full_params(amd_lib, STREAM, None), [(codes[at:at + n], lin[at:at + n]) for at, n in cuts_of(len(codes))])
    assert len(out) == 4 and any(w["segs"] for w in out)
    a.close()
    b.close()


def test_stream_s24_stereo_is_its_f32_twin(wrs, amd_lib, ctx, dev):
    """48 kHz stereo S24 read where it lies in device memory - two copies one byte apart, taken in turn, so that packets start on every byte
    phase of a dword - against F32 holding v / 2^23"""
    n = 48000 * 2
    rng = np.random.default_rng(31)
    t = np.arange(n) / 48000.0
    sig = np.stack([0.4 * np.sin(2 * np.pi * 330.0 * t), 0.3 * np.sin(2 * np.pi * (400.0 + 90.0 * t) * t)], axis=1) + 0.002 * rng.standard_normal((n, 2))
    s = np.clip(np.rint(sig.reshape(-1) * 8388608.0), -2 ** 23, 2 ** 23 - 1).astype(np.int32)
    x, f = wrs.pack_s24(s), s.astype(np.float32) / np.float32(8388608.0)
    d0, d1 = dev.put(x, 0), None
    second = DeviceBuffer(x.nbytes + 16)
    d1 = second.put(x, 1)
    kw = dict(step_ms=1000, length_ms=4000, keep_ms=200, sample_rate=48000, channels=2)
    a, b = wrs.WhisperStream(ctx, format=S24, **kw), wrs.WhisperStream(ctx, format=F32, **kw)
    feeds, phases = [], set()
    for k, (at, m) in enumerate(cuts_of(n)):
        p = (d1 if k % 2 else d0) + 6 * at
        phases.add(p % 4)
        feeds.append(((p, m), f[2 * at:2 * (at + m)]))
    assert phases == {0, 1, 2, 3}
    out = run_pair(amd_lib, a, b, GS.full_params(amd_lib, STREAM, None), feeds)
    assert len(out) == 2
    a.close()
    b.close()
    second.free()


def test_vad_stream_alaw_is_its_int16_twin(wrs, amd_lib, ctx, vctx):
    """whisper_amd_stream_open_vad fed A-law at 8 kHz: the utterance list of its int16 twin"""
    pcm = GV.recording()[:16000 * 7][::2]
    codes = wrs.linear_to_alaw(K.to_i16(pcm))
    lin = wrs.alaw_to_linear(codes)
    assert np.abs(lin.astype(np.int32) - K.to_i16(pcm).astype(np.int32)).max() <= 512           # half of A-law's largest step
    a, b = wrs.WhisperVadStream(ctx, vctx, sample_rate=8000, channels=1, format=ALAW), wrs.WhisperVadStream(ctx, vctx, sample_rate=8000, channels=1, format=I16)
    fp = GV.full_params(amd_lib, "greedy", None)
    utt = []

    def drain():
        assert a.pending() == b.pending()
        while a.pending() > 0:
            assert a.step(fp) == 1 and b.step(fp) == 1
            ua, ub = a.utterance_info(), b.utterance_info()
            assert [ua[k] for k in ("start", "length", "start_cs", "end_cs", "split")] == [ub[k] for k in ("start", "length", "start_cs", "end_cs", "split")]
            same(a.window(), b.window(), "utterance %d" % len(utt))
            assert segs_of(a.state) == segs_of(b.state)
            utt.append((ua["start_cs"], ua["end_cs"]))

    for at in range(0, len(codes), 800):
        assert a.feed(codes[at:at + 800]) == b.feed(lin[at:at + 800])
        drain()
    assert a.flush() == b.flush()
    drain()
    same(a.probs(), b.probs(), "probabilities")
    assert len(utt) >= 2, utt
    a.close()
    b.close()


# ---- a WAV file, end to end ----
def wav_image(tag, ch, rate, bits, payload):
    """a RIFF/WAVE image with an odd-sized LIST chunk in front of the data: the samples start at an even offset that is no multiple of 4"""
    block = ch * bits // 8
    fmt = struct.pack("<HHIIHHH", tag, ch, rate, rate * block, block, bits, 0)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"LIST" + struct.pack("<I", 7) + b"INFOabc\0" + b"data" + struct.pack("<I", len(payload)) + payload
    return np.frombuffer(b"RIFF" + struct.pack("<I", len(body)) + body, np.uint8)


def long_result(c):
    out, lib = [], c.lib
    for i in range(lib.whisper_full_n_segments(c.ptr)):
        toks = [lib.whisper_full_get_token_data(c.ptr, i, j) for j in range(lib.whisper_full_n_tokens(c.ptr, i))]
        out.append(dict(t0=lib.whisper_full_get_segment_t0(c.ptr, i), t1=lib.whisper_full_get_segment_t1(c.ptr, i),
                        text=lib.whisper_full_get_segment_text(c.ptr, i), ids=[t.id for t in toks],
                        p=[int(v) for v in np.array([t.p for t in toks], np.float32).view(np.uint32)], tok_t0=[t.t0 for t in toks], tok_t1=[t.t1 for t in toks]))
    return out


def test_wav_file_end_to_end(wrs, amd_lib, fctx):
    """tools/channels_cases.py's two_speakers at 8 kHz, compressed to mu-law and wrapped in a WAV header: whisper_amd_wav_parse, then
    whisper_amd_full_long_audio (channel 0 as a mono file) and whisper_amd_full_long_channels (the stereo file) give the segments and times
    of the calls on the expanded int16"""
    stereo = K.at_8k_i16(K.two_speakers())
    fp = wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, vad_model_path=V.model_path())
    for ch, pcm in ((1, K.channel(stereo, 0)), (2, stereo)):
        codes = wrs.linear_to_ulaw(pcm)
        image = wav_image(7, ch, 8000, 8, codes.tobytes())
        w = wrs.wav_parse(amd_lib, image)
        assert w == dict(data_offset=12 + 8 + 18 + 8 + 8 + 8, n_frames=len(codes) // ch, channels=ch, sample_rate=8000, format=ULAW, bits=8)
        assert w["data_offset"] % 4 == 2
        data = image[w["data_offset"]:w["data_offset"] + w["n_frames"] * ch]
        lin = wrs.ulaw_to_linear(codes)
        if ch == 1:
            assert fctx.full_long_audio(fp, lin, 1, 8000, I16) == 0
            want = long_result(fctx)
            assert fctx.full_long_audio(fp, data, w["channels"], w["sample_rate"], w["format"]) == 0
            got = long_result(fctx)
        else:
            assert fctx.full_long_channels(fp, lin, 8000, I16) == 0
            want = (long_result(fctx), fctx.segment_channels())
            assert fctx.full_long_channels(fp, data, w["sample_rate"], w["format"]) == 0
            got = (long_result(fctx), fctx.segment_channels())
            assert set(got[1]) == {0, 1}
        assert want and got == want, ch
    # the parser's refusals reach the caller as codes
    for bad, rc in ((b"RF64" + bytes(image[4:]), -2), (bytes(image[:40]), -3), (bytes(image[:38]), -5), (b"", -1)):
        with pytest.raises(wrs.WhisperError) as e:
            wrs.wav_parse(amd_lib, bad)
        assert e.value.code == rc


# ---- refusals ----
def test_refusals(wrs, amd_lib, ctx, fctx, vctx):
    """formats 2, 9 and -1 at every entry, and three channels with a new format; a refused call leaves the last result and the counters standing"""
    lib = amd_lib
    st = ctx.create_state()
    x, v = make_input(wrs, np.random.default_rng(7), 3000 * 2, ULAW)
    st.audio_to_pcm(x, 2, 8000, ULAW)
    st.audio_split(x, 8000, ULAW)
    want, planes = st.audio_copy(), [st.audio_split_copy(c) for c in (0, 1)]
    data, n, stride = C.c_void_p(x.ctypes.data), C.c_int64(-77), C.c_int64(-77)
    fp = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    lp = wrs.FullParams(lib, best_of=1, temperature_inc=0.0, vad_model_path=V.model_path())
    cp = wrs.whisper_amd_channels_params()
    lib.whisper_amd_channels_default_params(C.byref(cp))
    for fmt in (2, 9, -1):
        assert not lib.whisper_amd_audio_to_pcm(st.ptr, data, 100, 2, 8000, fmt, C.byref(n)) and n.value == -77
        assert lib.whisper_amd_full_audio(ctx.ptr, st.ptr, fp.c, data, 100, 2, 8000, fmt) == -1
        assert lib.whisper_amd_full_long_audio(fctx.ptr, lp.c, data, 100, 2, 8000, fmt, 0, 0) == -1
        assert not lib.whisper_amd_audio_split(st.ptr, data, 100, 8000, fmt, C.byref(n), C.byref(stride)) and (n.value, stride.value) == (-77, -77)
        assert lib.whisper_amd_full_long_channels(fctx.ptr, lp.c, C.byref(cp), data, 100, 8000, fmt) == -1
        with pytest.raises(wrs.WhisperError):
            wrs.WhisperStream(ctx, sample_rate=8000, channels=1, format=fmt)
        with pytest.raises(wrs.WhisperError):
            wrs.WhisperVadStream(ctx, vctx, sample_rate=8000, channels=1, format=fmt)
    for fmt in NEW:
        assert not lib.whisper_amd_audio_to_pcm(st.ptr, data, 100, 3, 8000, fmt, C.byref(n)) and n.value == -77
        assert lib.whisper_amd_full_audio(ctx.ptr, st.ptr, fp.c, data, 100, 3, 8000, fmt) == -1
        with pytest.raises(wrs.WhisperError):
            wrs.WhisperStream(ctx, sample_rate=8000, channels=3, format=fmt)
    same(st.audio_copy(), want, "after the refusals")
    for c in (0, 1):
        same(st.audio_split_copy(c), planes[c], "plane %d after the refusals" % c)
    assert st.audio_stats() == (1, 0, 0)
    st.free()


if __name__ == "__main__" and "--child" in sys.argv:
    child_main()

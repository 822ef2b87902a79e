"""The audio front end's kernels (whisper-rust_amd/csrc/wa_audio.hip) against wa_audio_ref, the host restatement of wa_audio.h, bit for bit.

Through tests/native/libaudio_kernels.so (the launcher of the product's own wa_audio_k.o on a device copy of the input, with guard values on
both sides of the output) and through the C ABI on a state (whisper_amd_audio_to_pcm with host and with device pointers).  The restatement
itself is held to float64 by tests/test_audio_math.py, which also shows that a wrong phase, reversed taps or a wrong first frame change these
expected values.  Lengths: 1, K/2 - 1, K, three tiles' worth of input plus 17, and the inputs that give tile - 1, tile and tile + 1 outputs."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import wsynth
from conftest import ROOT

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(ROOT, "tests", "native", "libaudio_kernels.so")
RATES = [8000, 11025, 16000, 22050, 44100, 48000, 96000]
I16, F32 = 0, 1
COMBOS = [(I16, 1), (I16, 2), (F32, 1), (F32, 2)]


def plan_of(rate):
    g = math.gcd(rate, 16000)
    L, M = 16000 // g, rate // g
    return L, M, 0 if rate == 16000 else 64 * -(-max(L, M) // L)


def n_out_of(n_frames, rate):
    return -(-n_frames * 16000 // rate)


def frames_for(n_out, rate):
    """the shortest input that gives n_out samples - at least n_out below 16 kHz, where not every count occurs (8 kHz gives even counts only)"""
    n = (n_out - 1) * rate // 16000 + 1
    assert n_out_of(n, rate) >= n_out and (n == 1 or n_out_of(n - 1, rate) < n_out) and (rate < 16000 or n_out_of(n, rate) == n_out)
    return n


def lengths_of(rate, tile):
    K = plan_of(rate)[2] or 64
    return [1, K // 2 - 1, K, frames_for(3 * tile, rate) + 17, frames_for(tile - 1, rate) - 1, frames_for(tile - 1, rate), frames_for(tile, rate), frames_for(tile + 1, rate)]


def random_input(rng, n_frames, ch, fmt):
    n = n_frames * ch
    if fmt == I16:
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[:min(n, 6)] = np.array([32767, -32768, -32767, 32767, -32768, -32768], np.int16)[:min(n, 6)]
        return x
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    x[:min(n, 4)] = np.array([1.0, 1.0, -1.0, -1.0], np.float32)[:min(n, 4)]
    return x


def square_input(n_frames, ch, fmt, period=37):
    """full scale, the two channels in step: +max for `period` frames, then -max"""
    s = np.where((np.arange(n_frames) // period) % 2 == 0, 1, -1)
    x = np.repeat(s, ch)
    return np.where(x > 0, 32767, -32768).astype(np.int16) if fmt == I16 else x.astype(np.float32)


def impulse_input(n_frames, ch, fmt, spacing):
    """single full-scale impulses `spacing` frames apart, of alternating sign, on both channels; the frames that carry one"""
    at = np.arange(spacing // 2, n_frames, spacing)
    s = np.zeros(n_frames, np.int64)
    s[at] = np.where(np.arange(len(at)) % 2 == 0, 1, -1)
    x = np.repeat(s, ch)
    return (np.where(x > 0, 32767, np.where(x < 0, -32768, 0)).astype(np.int16) if fmt == I16 else x.astype(np.float32)), at


class Harness:
    def __init__(self):
        self.lib = C.CDLL(HARNESS)
        self.lib.atest_n_out.restype = C.c_longlong
        self.lib.atest_n_out.argtypes = [C.c_longlong, C.c_int]
        self.lib.atest_ref.restype = C.c_longlong
        self.lib.atest_ref.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_void_p]
        self.lib.atest_run.restype = C.c_longlong
        self.lib.atest_run.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        self._ref = {}

    def ref(self, x, n_frames, ch, rate, fmt):
        key = (x.tobytes(), n_frames, ch, rate, fmt)
        if key not in self._ref:
            n = self.lib.atest_n_out(n_frames, rate)
            assert n == n_out_of(n_frames, rate)
            out = np.full(max(n, 1), np.nan, np.float32)
            assert self.lib.atest_ref(x.ctypes.data, n_frames, ch, rate, fmt, out.ctypes.data) == n
            self._ref[key] = out[:n]
        return self._ref[key]

    def run(self, x, n_frames, ch, rate, fmt, offset=0):
        n = n_out_of(n_frames, rate)
        out = np.full(max(n, 1), np.nan, np.float32)
        r = self.lib.atest_run(x.ctypes.data, n_frames, ch, rate, fmt, offset, out.ctypes.data)
        assert r == n, "atest_run returned %d (-2 HIP error, -3 shape not taken, -4 a write outside the output)" % r
        return out[:n]


@pytest.fixture(scope="module")
def har():
    assert os.path.exists(HARNESS), "tests/native/libaudio_kernels.so is not built (whisper-rust_amd/Makefile: audio_harness)"
    return Harness()


@pytest.fixture(scope="module")
def tile(amd_lib):
    t = amd_lib.whisper_amd_audio_tile()
    assert t >= 256 and t % 256 == 0
    return t


def same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: %d of %d samples differ, first at %d: %r != %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("rate", RATES)
def test_kernel_is_the_restatement_random(har, tile, rate):
    """every format, channel count and length; the device input 16-byte aligned and one sample behind a 16-byte boundary"""
    rng = np.random.default_rng(77 + rate)
    for fmt, ch in COMBOS:
        for n in lengths_of(rate, tile):
            x = random_input(rng, n, ch, fmt)
            want = har.ref(x, n, ch, rate, fmt)
            assert np.all(np.isfinite(want))
            for off in (0, 2 if fmt == I16 else 4):
                same(har.run(x, n, ch, rate, fmt, off), want, "rate %d fmt %d ch %d n %d offset %d" % (rate, fmt, ch, n, off))


@pytest.mark.parametrize("rate", RATES)
def test_kernel_is_the_restatement_square_wave(har, tile, rate):
    n = frames_for(2 * tile, rate) + 17
    for fmt, ch in COMBOS:
        x = square_input(n, ch, fmt)
        want = har.ref(x, n, ch, rate, fmt)
        same(har.run(x, n, ch, rate, fmt), want, "rate %d fmt %d ch %d" % (rate, fmt, ch))
        if rate != 16000:
            assert np.abs(want).max() > 1.0             # the overshoot of a band-limited edge: nothing clips or saturates


@pytest.mark.parametrize("rate,n_frames", [(11025, 2000), (44100, 3000)])
def test_impulses_reach_every_phase(har, tile, rate, n_frames):
    """Impulses more than K frames apart: every output sees at most one, so it is one tap times one sample; together they pass through every phase
    of the table (L = 640 at 11025 Hz, 160 at 44100 Hz)."""
    L, M, K = plan_of(rate)
    for fmt, ch in ((I16, 2), (F32, 1)):
        x, at = impulse_input(n_frames, ch, fmt, K + 1)
        want = har.ref(x, n_frames, ch, rate, fmt)
        same(har.run(x, n_frames, ch, rate, fmt), want, "rate %d fmt %d ch %d" % (rate, fmt, ch))
        n = np.arange(len(want), dtype=np.int64)
        first = n * M // L - K // 2 + 1                                     # the window of output n: frames first .. first + K - 1
        nxt = np.searchsorted(at, first)
        hit = (nxt < len(at)) & (at[np.minimum(nxt, len(at) - 1)] < first + K)
        assert set(((n * M) % L)[hit].tolist()) == set(range(L))
        assert np.count_nonzero(want[hit]) > len(want) // 2


# ---- through the C ABI, on a state ----
@pytest.fixture(scope="module")
def ctx(wrs, amd_lib):
    c = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, gpu_device=0), lib=amd_lib)
    yield c
    c.free()


class DeviceCopy:
    """a device copy of a host array, `offset` bytes behind a 256-byte boundary"""
    def __init__(self, x, offset=0):
        self.hip = C.CDLL("libamdhip64.so")
        self.base = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.base), C.c_size_t(x.nbytes + 512)) == 0
        self.ptr = self.base.value + offset
        assert self.hip.hipMemcpy(C.c_void_p(self.ptr), C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0

    def free(self):
        self.hip.hipFree(self.base)


@pytest.mark.parametrize("rate", RATES)
def test_to_pcm_host_and_device_pointers(wrs, har, tile, ctx, rate):
    """the same lengths, formats and channel counts through whisper_amd_audio_to_pcm: input in host memory, in device memory, and in device
    memory one sample behind a 16-byte boundary"""
    rng = np.random.default_rng(5 + rate)
    st = ctx.create_state()
    calls = 0
    for n in lengths_of(rate, tile):
        for fmt, ch in COMBOS:
            x = random_input(rng, n, ch, fmt)
            want = har.ref(x, n, ch, rate, fmt)
            ptr, got_n = st.audio_to_pcm(x, ch, rate)
            assert ptr and got_n == len(want) == st.lib.whisper_amd_audio_n_samples(n, rate)
            same(st.audio_copy(), want, "host pointer, rate %d fmt %d ch %d n %d" % (rate, fmt, ch, n))
            for off in (0, 2 if fmt == I16 else 4):
                d = DeviceCopy(x, off)
                ptr2, got_n = st.audio_to_pcm((d.ptr, n), ch, rate, fmt)
                assert ptr2 == ptr and got_n == len(want)                  # the state's buffer, not grown by an equal length
                same(st.audio_copy(), want, "device pointer + %d, rate %d fmt %d ch %d n %d" % (off, rate, fmt, ch, n))
                d.free()
            calls += 3
    assert st.audio_stats() == (calls, 0, 0)
    st.free()


def test_buffer_reuse(wrs, har, tile, ctx):
    """a long call, then a short one on the same state: the short result is the restatement's whatever the buffer held"""
    rng = np.random.default_rng(11)
    st = ctx.create_state()
    for rate in (44100, 16000):
        n_long, n_short = frames_for(5 * tile, rate) + 3, frames_for(tile, rate) - 5
        xl, xs = random_input(rng, n_long, 2, I16), random_input(rng, n_short, 2, I16)
        p1, n1 = st.audio_to_pcm(xl, 2, rate)
        same(st.audio_copy(), har.ref(xl, n_long, 2, rate, I16), "long")
        p2, n2 = st.audio_to_pcm(xs, 2, rate)
        assert p2 == p1 and n2 < n1
        same(st.audio_copy(), har.ref(xs, n_short, 2, rate, I16), "short after long, rate %d" % rate)
    p0, n0 = st.audio_to_pcm(np.zeros(0, np.int16), 1, 48000)
    assert p0 and n0 == 0 and len(st.audio_copy()) == 0                 # no frames: no samples, and still a pointer
    st.free()


def test_host_path_is_the_same(wrs, har, tile, ctx, monkeypatch):
    """WHISPER_AMD_AUDIO_HOST=1 when the state is created: the restatement serves the call, with a host and with a device pointer"""
    monkeypatch.setenv("WHISPER_AMD_AUDIO_HOST", "1")
    st = ctx.create_state()
    monkeypatch.delenv("WHISPER_AMD_AUDIO_HOST")
    rng = np.random.default_rng(12)
    n = frames_for(tile, 22050) + 1
    x = random_input(rng, n, 2, F32)
    want = har.ref(x, n, 2, 22050, F32)
    st.audio_to_pcm(x, 2, 22050)
    same(st.audio_copy(), want, "host path, host pointer")
    d = DeviceCopy(x, 4)
    st.audio_to_pcm((d.ptr, n), 2, 22050, F32)
    same(st.audio_copy(), want, "host path, device pointer")
    d.free()
    assert st.audio_stats() == (0, 2, 0)
    st.free()


def test_refusals(wrs, amd_lib, har, tile, ctx):
    st = ctx.create_state()
    rng = np.random.default_rng(13)
    x = random_input(rng, 3000, 2, I16)
    want = har.ref(x, 3000, 2, 48000, I16)
    st.audio_to_pcm(x, 2, 48000)
    lib, n = amd_lib, C.c_int64(-77)
    data = C.c_void_p(x.ctypes.data)
    bad = [(None, 10, 2, 48000, I16), (data, -1, 2, 48000, I16), (data, 100, 0, 48000, I16), (data, 100, 3, 48000, I16), (data, 100, -2, 48000, I16),
           (data, 100, 2, 48000, 2), (data, 100, 2, 48000, -1), (data, 100, 2, 7999, I16), (data, 100, 2, 192001, I16), (data, 100, 2, 16001, I16),
           (data, 100, 2, 0, I16), (data, 100, 2, -48000, I16)]
    fp = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    for d, nf, ch, rate, fmt in bad:
        assert not lib.whisper_amd_audio_to_pcm(st.ptr, d, nf, ch, rate, fmt, C.byref(n)), (nf, ch, rate, fmt)
        assert n.value == -77
        assert lib.whisper_amd_full_audio(ctx.ptr, st.ptr, fp.c, d, nf, ch, rate, fmt) == -1
    assert not lib.whisper_amd_audio_to_pcm(None, data, 100, 2, 48000, I16, C.byref(n))
    assert not lib.whisper_amd_audio_to_pcm(st.ptr, data, 100, 2, 48000, I16, None)
    for rate in (7999, 192001, 16001, 0):
        assert lib.whisper_amd_audio_n_samples(100, rate) == -1 and lib.whisper_amd_audio_taps(rate, None, 0, None, None, None) == -1
    assert lib.whisper_amd_audio_n_samples(-1, 48000) == -1
    # nothing was written: the last result and the counters stand, and the state still works
    same(st.audio_copy(), want, "after the refusals")
    assert st.audio_stats() == (1, 0, 0)
    st.audio_to_pcm(x[:2000], 1, 11025)
    same(st.audio_copy(), har.ref(x[:2000], 2000, 1, 11025, I16), "a call after the refusals")
    fresh = ctx.create_state()
    assert lib.whisper_amd_audio_copy(fresh.ptr, None, 0) == -1         # no result yet
    fresh.free()
    st.free()


def test_taps_entry_is_the_table_the_kernels_use(wrs, amd_lib, har):
    """whisper_amd_audio_taps: one impulse of 1.0 at frame i reads the table back through the kernel, tap by tap"""
    for rate in (44100, 8000):
        t, L, M, K = wrs.audio_taps(amd_lib, rate)
        assert (L, M, K) == plan_of(rate) and t.shape == (L, K)
        n_frames, i = 4 * K, 2 * K
        x = np.zeros(n_frames, np.float32)
        x[i] = 1.0
        y = har.run(x, n_frames, 1, rate, F32)
        n = np.arange(len(y), dtype=np.int64)
        k = i - (n * M // L - K // 2 + 1)
        ok = (k >= 0) & (k < K)
        want = np.where(ok, t[(n * M) % L, np.clip(k, 0, K - 1)], np.float32(0.0)).astype(np.float32)
        same(y, want, "rate %d" % rate)
    assert wrs.audio_taps(amd_lib, 16000)[0].size == 0

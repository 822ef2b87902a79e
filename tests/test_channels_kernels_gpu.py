"""The two-channel kernels (whisper-rust_amd/csrc/wa_channels.hip) against the host restatements of wa_channels.h, bit for bit.

Through tests/native/libchannels_kernels.so: the launchers of the product's own wa_channels_k.o on device copies, with a mark on both sides of
the planar output and between a plane's end and its stride.  The restatements themselves are held to wa_audio_ref per channel, to integer
arithmetic and to a sequential float64 sum by tests/test_channels_math.py.
Split: int16 and F32 at 16 000, 8 000, 44 100 and 48 000 Hz (16 kHz: k_audio_deinterleave; 8 and 48 kHz: k_audio_split with the taps in LDS;
44.1 kHz: taps in global memory); 0, 1, 2, 7, 8, 9 frames and the inputs that give tile - 1, tile, tile + 1 and 2 tile + 3 outputs; the device
input 16-byte aligned and one frame behind a 16-byte boundary (the scalar loads); the channels are independent draws.
Energy: empty, one-sample, unaligned and lane-edge spans, one span of 480 000 samples, 1, 2 and 257 spans in one launch."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(ROOT, "tests", "native", "libchannels_kernels.so")
RATES = [16000, 8000, 44100, 48000]
I16, F32 = 0, 1


def n_out_of(n_frames, rate):
    return -(-n_frames * 16000 // rate)


def frames_for(n_out, rate):
    """the shortest input that gives at least n_out samples (8 kHz gives even counts only)"""
    return (n_out - 1) * rate // 16000 + 1


def make_stereo(rng, n_frames, fmt):
    if fmt == I16:
        x = rng.integers(-32768, 32768, 2 * n_frames).astype(np.int16)
        x[:min(len(x), 4)] = np.array([32767, -32768, -32768, 32767], np.int16)[:min(len(x), 4)]
        return x
    return rng.uniform(-1.0, 1.0, 2 * n_frames).astype(np.float32)


class Harness:
    def __init__(self):
        L = self.lib = C.CDLL(HARNESS)
        LL, P, I = C.c_longlong, C.c_void_p, C.c_int
        L.ctest_n_out.restype = LL; L.ctest_n_out.argtypes = [LL, I]
        L.ctest_stride.restype = LL; L.ctest_stride.argtypes = [LL]
        L.ctest_split_ref.restype = LL; L.ctest_split_ref.argtypes = [P, LL, I, I, P]
        L.ctest_split_run.restype = LL; L.ctest_split_run.argtypes = [P, LL, I, I, I, P]
        L.ctest_energy_ref.restype = None; L.ctest_energy_ref.argtypes = [P, LL, LL, P, I, P]
        L.ctest_energy_run.restype = I; L.ctest_energy_run.argtypes = [P, LL, LL, P, I, P]

    def shape(self, n_frames, rate):
        n = self.lib.ctest_n_out(n_frames, rate)
        assert n == n_out_of(n_frames, rate)
        stride = self.lib.ctest_stride(n)
        assert stride >= n and stride % 64 == 0 and stride - n < 64
        return n, stride

    def split_ref(self, x, n_frames, rate, fmt):
        n, stride = self.shape(n_frames, rate)
        out = np.full(max(2 * stride, 1), np.nan, np.float32)
        assert self.lib.ctest_split_ref(x.ctypes.data, n_frames, rate, fmt, out.ctypes.data) == n
        return out[:n], out[stride:stride + n]

    def split_run(self, x, n_frames, rate, fmt, offset=0):
        n, stride = self.shape(n_frames, rate)
        out = np.full(max(2 * stride, 1), np.nan, np.float32)
        r = self.lib.ctest_split_run(x.ctypes.data, n_frames, rate, fmt, offset, out.ctypes.data)
        assert r == n, "ctest_split_run returned %d (-2 HIP error, -3 shape not taken, -4 a write outside the planes)" % r
        return out[:n], out[stride:stride + n]

    def energy(self, planes, n, stride, spans, run):
        s = np.ascontiguousarray(spans, dtype=np.int64).reshape(-1)
        e = np.full(max(len(s), 1), np.nan, np.float64)
        if run:
            assert self.lib.ctest_energy_run(planes.ctypes.data, n, stride, s.ctypes.data, len(s) // 2, e.ctypes.data) == 0
        else:
            self.lib.ctest_energy_ref(planes.ctypes.data, n, stride, s.ctypes.data, len(s) // 2, e.ctypes.data)
        return e[:len(s)].reshape(-1, 2)


@pytest.fixture(scope="module")
def har():
    assert os.path.exists(HARNESS), "tests/native/libchannels_kernels.so is not built (whisper-rust_amd/Makefile: channels_harness)"
    return Harness()


@pytest.fixture(scope="module")
def tile(amd_lib):
    t = amd_lib.whisper_amd_channels_tile()
    assert t >= 256 and t % 256 == 0
    return t


def same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: %d of %d samples differ, first at %d: %r != %r" % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def lengths_of(rate, tile):
    return [0, 1, 2, 7, 8, 9] + [frames_for(k, rate) for k in (tile - 1, tile, tile + 1, 2 * tile + 3)]


@pytest.mark.parametrize("rate", RATES)
def test_split_is_the_restatement(har, tile, rate):
    rng = np.random.default_rng(91 + rate)
    for fmt in (I16, F32):
        for n in lengths_of(rate, tile):
            x = make_stereo(rng, n, fmt)
            w0, w1 = har.split_ref(x, n, rate, fmt)
            assert np.all(np.isfinite(w0)) and np.all(np.isfinite(w1))
            if len(w0) > 4:
                assert not np.array_equal(w0, w1)                # independent draws: a swapped or mixed channel shows below
            for off in (0, 4 if fmt == I16 else 8):
                g0, g1 = har.split_run(x, n, rate, fmt, off)
                same(g0, w0, "plane 0, rate %d fmt %d n %d offset %d" % (rate, fmt, n, off))
                same(g1, w1, "plane 1, rate %d fmt %d n %d offset %d" % (rate, fmt, n, off))


@pytest.mark.parametrize("rate", RATES)
def test_a_silent_channel_is_plus_zero(har, tile, rate):
    rng = np.random.default_rng(17 + rate)
    n = frames_for(tile + 1, rate) + 5
    for fmt in (I16, F32):
        x = make_stereo(rng, n, fmt)
        x[1::2] = 0
        g0, g1 = har.split_run(x, n, rate, fmt)
        w0, w1 = har.split_ref(x, n, rate, fmt)
        same(g0, w0, "plane 0, rate %d fmt %d" % (rate, fmt))
        assert not g1.view(np.uint32).any(), "plane 1 is not +0.0 everywhere (rate %d fmt %d)" % (rate, fmt)
        assert g0.view(np.uint32).any()


# ---- energy ----
N = 480000 + 777


@pytest.fixture(scope="module")
def planes(har):
    """two planes `stride` apart: random N(0, 0.1), the channels different"""
    rng = np.random.default_rng(3)
    stride = har.lib.ctest_stride(N)
    p = np.zeros(2 * stride, np.float32)
    p[:N] = rng.normal(0.0, 0.1, N)
    p[stride:stride + N] = rng.normal(0.0, 0.3, N)
    return p, stride


def edge_spans(lanes):
    return [(0, 0), (9, 3), (5, 6), (0, 1), (N - 1, N), (3, lanes), (3, lanes - 1), (3, lanes + 1), (lanes, 2 * lanes), (lanes - 1, 3 * lanes + 7),
            (-50, 40), (N - 40, N + 1000), (N, N + 5), (777, 480777), (0, N)]


def test_energy_is_the_restatement(har, amd_lib, planes):
    p, stride = planes
    lanes = amd_lib.whisper_amd_channels_energy_lanes()
    assert lanes == 256
    spans = edge_spans(lanes)
    assert any(b - a == 480000 for a, b in spans)
    want = har.energy(p, N, stride, spans, run=False)
    got = har.energy(p, N, stride, spans, run=True)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    assert np.all(want[:2] == 0.0) and not np.signbit(got[:2]).any() and np.all(got[12] == 0.0)
    assert want[2, 0] == float(abs(p[5])) and want[2, 1] == float(abs(p[stride + 5]))
    assert np.all(want[-1] > 0) and want[-1, 1] > 2 * want[-1, 0]               # the channels are not confused


@pytest.mark.parametrize("n_spans", [1, 2, 257])
def test_energy_many_spans_in_one_launch(har, planes, n_spans):
    p, stride = planes
    rng = np.random.default_rng(40 + n_spans)
    a = rng.integers(-100, N, n_spans)
    spans = [(int(s), int(s + l)) for s, l in zip(a, rng.integers(0, 5000, n_spans))]
    want = har.energy(p, N, stride, spans, run=False)
    got = har.energy(p, N, stride, spans, run=True)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    one_by_one = np.concatenate([har.energy(p, N, stride, [s], run=True) for s in spans[:5]])       # a span's sum does not depend on its company
    assert np.array_equal(one_by_one.view(np.uint64), want[:5].view(np.uint64))


def test_energy_exact_on_dyadic_samples(har, amd_lib):
    """multiples of 2^-10 in [-1, 1]: every order gives the exact sum; the kernel against integer arithmetic"""
    rng = np.random.default_rng(77)
    stride = har.lib.ctest_stride(N)
    k = np.zeros(2 * stride, np.int64)
    k[:N] = rng.integers(-1024, 1025, N)
    k[stride:stride + N] = rng.integers(-1024, 1025, N)
    p = (k / 1024.0).astype(np.float32)
    spans = edge_spans(amd_lib.whisper_amd_channels_energy_lanes())
    got = har.energy(p, N, stride, spans, run=True)
    for (a, b), e in zip(spans, got):
        a, b = max(a, 0), min(b, N)
        for c in range(2):
            want = int(np.abs(k[c * stride + a:c * stride + b]).sum()) if a < b else 0
            assert e[c] * 1024.0 == want, (a, b, c, e[c], want)

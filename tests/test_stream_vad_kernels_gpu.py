"""k_stream_vad_front (whisper-rust_amd/csrc/wa_vad.hip): the VAD front end on the ring windows of several live sessions in one launch, held
to whisper_amd_vad_front - k_vad_front, which tests/test_vad_gpu.py pins to the reference - on the same samples laid out linearly, bit for bit.

Through tests/native/libstream_vad_kernels.so: the launcher of the product's own wa_vad_k.o, with the synthetic model's tensors uploaded in
the product's layout.  Rings of 4100 samples (no multiple of 512: windows straddle the wrap) and of other sizes, starting 0, 4, 8 and 12 bytes
behind a 16-byte boundary; 1, 7, 8 and 9 windows of one session; 1, 3 and 8 sessions with unequal counts, one of them zero (8 sessions of 3
windows: three workgroups); a last window with 1 and with 511 valid samples.  Every ring slot that holds no sample of the launch is NaN, so
is everything around a ring and around a session's output rows: a read past the valid samples shows in the result, a write outside the rows
in the guards, and the rings are compared with what was uploaded.  (That the code object shows no scratch and no spilled register is read
from the build tree, where it is: tests/test_stream_vad_math.py.)"""
import ctypes as C
import os

import numpy as np
import pytest

import wsynth_vad as V
from conftest import ROOT

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(ROOT, "tests", "native", "libstream_vad_kernels.so")
G = 64
W = 512


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def harness():
    h = C.CDLL(HARNESS)          # no fallback: a missing harness is a failure of the build
    t = dict(V.tensors())
    u16 = lambda name: np.ascontiguousarray(t[name]).view(np.uint16).reshape(-1)
    f32 = lambda name: np.ascontiguousarray(t[name], np.float32).reshape(-1)
    arrs = [u16("_model.stft.forward_basis_buffer")] + [u16("_model.encoder.%d.reparam_conv.weight" % i) for i in range(4)] + \
           [f32("_model.encoder.%d.reparam_conv.bias" % i) for i in range(4)] + [f32("_model.decoder.rnn.weight_ih"), f32("_model.decoder.rnn.bias_ih")]
    assert [a.size for a in arrs] == [258 * 256, 128 * 387, 64 * 384, 64 * 192, 128 * 192, 128, 64, 64, 128, 512 * 128, 512]
    h.svtest_set_weights.argtypes = [C.c_void_p] * 11
    assert h.svtest_set_weights(*[a.ctypes.data for a in arrs]) == 0
    h.svtest_run.argtypes = [C.c_int] + [C.c_void_p] * 7 + [C.c_longlong]
    h.keep = arrs
    return h


@pytest.fixture(scope="module")
def vad(wrs, amd_lib):
    v = wrs.WhisperVadContext.new(V.model_path(), lib=amd_lib)
    yield v
    v.free()


@pytest.fixture(scope="module")
def audio():
    return V.synth_audio()           # 14 s: bursts of tone and chirp, faint noise between them


def run(h, vad, sessions):
    """sessions: [(samples, cap, slot, ring_off)]; the launch against the whole-recording front end on each session's samples"""
    n = len(sessions)
    n_samples = np.asarray([len(s[0]) for s in sessions], np.int32)
    n_windows = np.asarray([-(-len(s[0]) // W) for s in sessions], np.int32)
    cap, slot, off = (np.asarray([s[k] for s in sessions], np.int32) for k in (1, 2, 3))
    flat = np.ascontiguousarray(np.concatenate([np.asarray(s[0], np.float32) for s in sessions] + [np.zeros(1, np.float32)]))
    row = 2 * G + W * max(int(n_windows.max()), 1) + 4
    out = np.zeros((n, row), np.float32)
    rc = h.svtest_run(n, flat.ctypes.data, n_samples.ctypes.data, n_windows.ctypes.data, cap.ctypes.data, slot.ctypes.data, off.ctypes.data, out.ctypes.data, row)
    assert rc == 0, rc
    for i, s in enumerate(sessions):
        nw = int(n_windows[i])
        assert np.all(np.isnan(out[i, :G])) and np.all(np.isnan(out[i, G + W * nw:])), ("guards of session", i)
        if nw == 0:
            continue
        want = vad.front(np.ascontiguousarray(s[0], np.float32))
        assert want.shape == (nw, W)
        got = out[i, G:G + W * nw].reshape(nw, W)
        assert not np.any(np.isnan(got)), ("a sample outside the valid ones was read", i)
        assert np.array_equal(bits(got), bits(want)), ("session", i, np.argwhere(bits(got) != bits(want))[:4])


def test_constants(harness):
    assert harness.svtest_sessions() == 8 and harness.svtest_max_windows() >= 1024


@pytest.mark.parametrize("n_windows", [1, 7, 8, 9])
@pytest.mark.parametrize("off", [0, 1, 2, 3])
def test_one_session_across_the_wrap(harness, vad, audio, n_windows, off):
    """a ring of 4100 samples, the first window starting 300 samples before its end: the first window wraps inside itself, at a slot that is
    no multiple of 4"""
    a = audio[16000:16000 + n_windows * W]
    run(harness, vad, [(a, 4100 if n_windows <= 8 else 4700, 4100 - 301, off)])


@pytest.mark.parametrize("valid", [1, 511])
def test_partial_last_window(harness, vad, audio, valid):
    a = audio[17000:17000 + 2 * W + valid]
    run(harness, vad, [(a, 4100, 3000, 1)])
    run(harness, vad, [(audio[17000:17000 + valid], 4100, 4099, 3)])


@pytest.mark.parametrize("n_sessions", [1, 3, 8])
def test_several_sessions_unequal_counts(harness, vad, audio, n_sessions):
    counts = {1: [5], 3: [3, 0, 9], 8: [1, 4, 0, 8, 2, 9, 3, 7]}[n_sessions]
    sessions = []
    for i, c in enumerate(counts):
        start = 16000 + 9000 * i
        n = c * W - (37 if i == n_sessions - 1 and c else 0)           # the last session ends in a partial window
        sessions.append((audio[start:start + n], (4100 if c <= 8 else 4700) + 13 * i, (1700 * (i + 1)) % 4100, i % 4))
    run(harness, vad, sessions)


def test_eight_sessions_of_three_windows(harness, vad, audio):
    """24 windows: three workgroups, each with rows of three sessions"""
    run(harness, vad, [(audio[8000 * i + 4000:8000 * i + 4000 + 3 * W], 4100, (511 * (i + 3)) % 4100, (i + 1) % 4) for i in range(8)])

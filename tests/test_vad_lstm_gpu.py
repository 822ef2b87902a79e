"""k_vad_lstm (whisper-rust_amd/csrc/wa_vad_lstm.hip) alone: whisper_amd_vad_recur on gate inputs and states of the test's making against the
product's host recurrence (wa_vad_step, through tests/native/vad_lstm_ref.cpp compiled by g++), bit for bit on the probabilities and on the
final h and c.  The model is the synthetic Silero-shaped one of tools/wsynth_vad.py.  The pre-activation of gate row j is gate_in[j] + (W_hh h + b_hh)[j].  From a zero h the bracket is b_hh[j] exactly, so gate inputs of
scale * noise - b_hh put the FIRST window's pre-activations at the chosen scale (the later windows of a case run on whatever state follows).
No F32 gate input can leave a sum below 2^-55 beside a bias of 0.1, so the "tiny" case cancels the bias exactly instead: the g rows' tanh sees
0, c becomes f * c0 with c0 around 2^-70 (one entry subnormal), and tanh(c) takes the branch below 2^-55."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT
import wsynth_vad as V

pytestmark = pytest.mark.gpu

FP = C.POINTER(C.c_float)
SUB = np.float32(1e-41)                                   # a subnormal


@pytest.fixture(scope="module")
def host_step(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vad_lstm") / "libvad_lstm_ref.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-mavx2", "-mf16c", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(ROOT, "tests", "native", "vad_lstm_ref.cpp"),
                           os.path.join(ROOT, "whisper-rust_amd", "csrc", "wa_vad_host.cpp"), "-o", so])
    lib = C.CDLL(so)
    lib.vad_lstm_ref.argtypes = [C.c_char_p, FP, C.c_int, FP, FP, FP]

    def run(gates, h, c):
        g = np.ascontiguousarray(gates, np.float32).reshape(-1, 512)
        h, c, p = np.array(h, np.float32), np.array(c, np.float32), np.zeros(len(g), np.float32)
        ptr = lambda a: a.ctypes.data_as(FP)
        assert lib.vad_lstm_ref(V.model_path().encode(), ptr(g), len(g), ptr(h), ptr(c), ptr(p)) == 0
        return p, h, c
    return run


@pytest.fixture(scope="module")
def vctx(wrs, amd_lib):
    v = wrs.WhisperVadContext.new(V.model_path(), lib=amd_lib)
    assert v.lstm_path() == 1, "the device recurrence is off on this host"
    yield v
    v.free()


def gates_of(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 512)).astype(np.float32)


def state_of(B, seed):                                    # non-zero, entry 5 of h and entry 9 of c subnormal
    rng = np.random.default_rng(seed)
    h, c = (0.5 * rng.standard_normal((B, 128))).astype(np.float32), rng.standard_normal((B, 128)).astype(np.float32)
    h[:, 5], c[:, 9] = SUB, -SUB
    return h, c


def same(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def check(vctx, host_step, gates, h0, c0):
    probs, h, c = vctx.recur(gates, h0, c0)
    for b, g in enumerate(gates):
        wp, wh, wc = host_step(g, h0[b], c0[b])
        assert same(probs[b], wp) and same(h[b], wh) and same(c[b], wc), ("sequence", b, len(g), same(probs[b], wp), same(h[b], wh))
    return probs, h, c


@pytest.mark.parametrize("n", [1, 2, 9])
def test_windows(vctx, host_step, n):
    check(vctx, host_step, [gates_of(n, 10 + n)], *state_of(1, 3))       # first window, state carry, the prefetch's end; subnormals in h, c


def test_split_over_two_calls(vctx, host_step):
    g, z = gates_of(9, 21), np.zeros((1, 128), np.float32)
    whole, h, c = check(vctx, host_step, [g], z, z)
    first, h1, c1 = vctx.recur([g[:4]], z, z)
    second, h2, c2 = vctx.recur([g[4:]], h1, c1)
    assert same(np.concatenate([first[0], second[0]]), whole[0]) and same(h2, h) and same(c2, c)


@pytest.mark.parametrize("lengths", [[3], [0, 5], [4, 0, 1, 7, 2, 9, 3, 5]])
def test_sequences_per_launch(vctx, host_step, lengths):
    h0, c0 = state_of(len(lengths), 30 + len(lengths))
    before = vctx.lstm_stats()
    _, h, c = check(vctx, host_step, [gates_of(n, 40 + i) for i, n in enumerate(lengths)], h0, c0)
    after = vctx.lstm_stats()
    assert after[0] - before[0] == 1 and after[1] - before[1] == sum(lengths), "one launch for all sequences"
    for b in [b for b, n in enumerate(lengths) if n == 0]:
        assert same(h[b], h0[b]) and same(c[b], c0[b]), "an empty sequence's state is untouched"


@pytest.mark.parametrize("scale", ["tiny", 0.5, 4.0, 30.0, "+100", "-100"])
def test_activation_branches(vctx, host_step, scale):
    b_hh = dict(V.tensors(0))["_model.decoder.rnn.bias_hh"].astype(np.float32)
    g = gates_of(3, 50)
    h0, c0 = np.zeros((1, 128), np.float32), np.zeros((1, 128), np.float32)
    if scale == "tiny":
        g[0] = -b_hh
        c0[0], c0[0, 9] = (np.random.default_rng(51).standard_normal(128) * 2.0 ** -70).astype(np.float32), SUB
    else:
        g[0] = (np.float32(float(scale)) if isinstance(scale, str) else np.float32(scale) * g[0]) - b_hh
    _, h, c = check(vctx, host_step, [g[:1]], h0, c0)
    # tiny: tanh(c) below 2^-55; -100: expf overflows, every sigmoid is exactly 0; +100: it underflows to a subnormal, every sigmoid is exactly 1
    facts = {"tiny": np.all(np.abs(c[0]) < 2.0 ** -55) and np.any(h[0] != 0), "-100": np.all(c[0] == 0) and np.all(h[0] == 0), "+100": np.all(c[0] == 1)}
    assert facts.get(scale, True), scale
    check(vctx, host_step, [g], h0, c0)

"""k_long_pack alone (whisper-rust_amd/csrc/wa_long.hip) through whisper_amd_long_pack: the kernel (where = 1) against the host function
wa_vad_filter_audio (where = 0) and against the numpy restatement of tools/long_ref.py, bit for bit and length for length, on segment lists
built to sit on the kernel's edges.  The input is a ramp of distinct non-zero values, so a misplaced sample shows.  Also: the VAD on a
device copy of the audio, read in place, gives the probabilities of the host-pointer call."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import long_ref as R
import wsynth
import wsynth_vad as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

G = json.load(open(os.path.join(GOLDEN, "vad.json")))
N = 9000                        # samples of the ramp: 56.25 cs


def ov_for(k):
    """a samples_overlap that gives exactly k overlap samples"""
    ov = (k + 0.5) / 16000.0
    assert R.overlap_samples(ov) == k
    return ov


@pytest.fixture(scope="module")
def fctx(wrs, amd_lib):
    c = wrs.WhisperFullContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    yield c
    c.free()


@pytest.fixture(scope="module")
def ramp():
    return np.arange(1, N + 1, dtype=np.float32)


def cases(tile):
    """name -> (segments cs, runs (first, count), samples_overlap, n_samples)"""
    out = {
        "one_segment_of_1cs":      ([(5, 6)], [(0, 1)], 0.1, N),
        "back_to_back":            ([(10, 20), (20, 30), (30, 31)], [(0, 3)], 0.1, N),
        "zero_length_last":        ([(10, 20), (25, 25)], [(0, 2)], 0.1, N),                # the second segment has no sample and is skipped
        "zero_length_inside":      ([(10, 20), (25, 25), (30, 40)], [(0, 3)], 0.0, N),      # ... its silence with it: the tail stays zero
        "last_reaches_the_end":    ([(10, 20), (30, 50)], [(0, 2)], 0.1, 50 * 160),         # counted to n - 1, copied to n: one sample is cut off
        "last_beyond_the_end":     ([(10, 20), (30, 60)], [(0, 2)], 0.1, 50 * 160 + 7),
        "start_beyond_the_end":    ([(10, 20), (70, 80)], [(0, 2)], 0.1, N),                # start clamped to n - 1: one sample, and a shorter length
        "eight_chunks":            ([(2 * i, 2 * i + 1 + (i % 3)) for i in range(1, 13)], [(0, 2), (2, 1), (3, 2), (5, 1), (6, 1), (7, 2), (9, 1), (10, 2)], 0.1, N),
    }
    # the first piece [0 cs, 20 cs) + overlap ends at tile - 1, tile, tile + 1; then silence, then a second piece that crosses the next tile edge
    for d in (-1, 0, 1):
        out["piece_edge_at_tile%+d" % d] = ([(0, 20), (22, 55)], [(0, 2)], ov_for(tile + d - 3200), N)
    # the second piece's destination at every residue mod 4 while its source start stays a multiple of 4: every source residue of a 4-sample group
    for r in range(4):
        out["dst_residue_%d" % r] = ([(3, 9), (12, 40)], [(0, 2)], ov_for(100 + r), N)
    return out


def check(c, pcm, segs, runs, ov, n, dev=None):
    want = [R.packed_audio(pcm[:n], segs[f:f + k], ov) for f, k in runs]
    got = {}
    for where in (1, 0):
        assert c.long_pack(dev if dev is not None else pcm[:n], segs, ov, runs, where) == 0
        assert c.lib.whisper_amd_long_n_chunks(c.ptr) == len(runs)
        s = c.long_stats()                  # of this call alone: the kernel path uploads a host recording once, the host path uploads none of it
        assert (s["path"], s["chunks"], s["h2d_bytes"]) == (where, len(runs), 4 * n if where == 1 and dev is None else 0)
        got[where] = [c.long_chunk_copy(i) for i in range(len(runs))]
        info = c.long_chunks()
        assert [(i["first"], i["count"], i["packed"]) for i in info] == [(f, k, len(w)) for (f, k), w in zip(runs, want)]
    for i, w in enumerate(want):
        for where in (1, 0):
            assert got[where][i].shape == w.shape, "chunk %d, where %d: length" % (i, where)
            assert np.array_equal(got[where][i].view(np.uint32), w.view(np.uint32)), "chunk %d, where %d" % (i, where)
    return want


def test_tile_constant(amd_lib):
    t = amd_lib.whisper_amd_long_tile()
    assert t % 4 == 0 and 3201 < t <= 5000, "the piece_edge cases put a 20 cs segment plus its overlap around one tile, inside a 9000-sample ramp"


@pytest.mark.parametrize("name", sorted(cases(4096)))
def test_pack_kernel_equals_host_function(amd_lib, fctx, ramp, name):
    segs, runs, ov, n = cases(amd_lib.whisper_amd_long_tile())[name]
    want = check(fctx, ramp, segs, runs, ov, n)
    if name == "zero_length_inside":
        assert len(want[0]) == 1600 + 1600 + 2 * 1600 and not want[0][-1600:].any() and want[0][:1600].all()
    if name == "last_reaches_the_end":
        assert len(want[0]) == 1600 + 1600 + 1600 + 3200 - 1 and want[0][-1] == ramp[50 * 160 - 2]
    if name == "start_beyond_the_end":
        assert len(want[0]) == 3200 + 1600 - (70 * 160 - (N - 1))        # the length counts that segment as negative: the first piece is cut
    if name.startswith("piece_edge"):
        assert len(want[0]) > amd_lib.whisper_amd_long_tile() + 1600


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_audio_at_every_base_residue(wrs, amd_lib, fctx, ramp, shift):
    """The caller's audio already in HBM, its base `shift` floats off a 16-byte boundary: 16-byte loads where the address allows, else scalar ones."""
    st = wrs.WhisperState(fctx, fctx.state_ptr())
    ptr, n = st.audio_to_pcm(ramp, 1, 16000)
    assert n == N and np.array_equal(st.audio_copy(), ramp)
    segs, runs, ov, _ = cases(amd_lib.whisper_amd_long_tile())["piece_edge_at_tile+1"]
    check(fctx, ramp[shift:], segs, runs, ov, N - shift, dev=(ptr + 4 * shift, N - shift))


def test_refused_arguments(fctx, ramp):
    assert fctx.long_pack(ramp, [(5, 6)], 0.1, [(0, 2)], 1) == -1          # a run past the list
    assert fctx.long_pack(ramp, [(5, 6)], 0.1, [(0, 1)], 2) == -1          # no such path
    assert fctx.lib.whisper_amd_long_n_chunks(fctx.ptr) >= 0


def test_vad_on_device_audio(wrs, amd_lib, fctx):
    """whisper_vad_detect_speech on a device copy of the audio: the host-pointer call's probabilities, and the recorded ones, bit for bit."""
    pcm = V.synth_audio()
    v = wrs.WhisperVadContext.new(V.model_path(), lib=amd_lib)
    try:
        host = [int(x) for x in v.detect_speech(pcm).view(np.uint32)]
        st = wrs.WhisperState(fctx, fctx.state_ptr())
        ptr, n = st.audio_to_pcm(pcm, 1, 16000)
        assert n == len(pcm)
        for n_dev in (len(pcm), 513):
            assert amd_lib.whisper_vad_detect_speech(v.ptr, C.cast(C.c_void_p(ptr), C.POINTER(C.c_float)), n_dev)
            dev = [int(x) for x in v.probs().view(np.uint32)]
            assert dev == G["probs"]["full" if n_dev == len(pcm) else "n513"]["bits"]
        assert host == G["probs"]["full"]["bits"]
    finally:
        v.free()


def test_vad_on_device_audio_across_slabs(wrs, amd_lib, fctx, monkeypatch):
    """Slabs of 100 windows: every slab starts inside the caller's buffer, at a multiple of 512 floats."""
    monkeypatch.setenv("WHISPER_AMD_VAD_SLAB", "100")
    pcm = V.synth_audio()
    v = wrs.WhisperVadContext.new(V.model_path(), lib=amd_lib)
    try:
        st = wrs.WhisperState(fctx, fctx.state_ptr())
        ptr, n = st.audio_to_pcm(pcm, 1, 16000)
        assert amd_lib.whisper_vad_detect_speech(v.ptr, C.cast(C.c_void_p(ptr), C.POINTER(C.c_float)), n)
        assert [int(x) for x in v.probs().view(np.uint32)] == G["probs"]["full"]["bits"]
    finally:
        v.free()

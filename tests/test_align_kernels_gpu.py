"""k_align_score (whisper-rust_amd/csrc/wa_align.hip) alone, through tests/native/libalign_kernels.so: the launcher of the product's own
wa_align_k.o on a device copy of the rows, NaN in front of the first row, between the rows and behind the last.

The cases are those of tests/test_align_math.py (tools/align_cases.py) and the yardstick is the same numpy float64: best_id and rank are
exact and equal to the host restatement's, plog / best_plog / p / best_p lie within 1 F32 ulp of the float64 value (the bound is derived in
test_align_math.py; the device may differ from the host restatement in the last F64 bit of an exp, so the two are not held to each other
bit for bit).  Two device runs of the same input give identical bytes.  Every case runs with the first row on a 16-byte boundary; the
packed rows of an odd vocabulary (ld = n_vocab = 51865: every other row 4 bytes off), ld = n_vocab + 3 and first rows 1..3 floats off a
boundary put head and tail of the kernel's 16-byte path at every position.  One more run goes through whisper_amd_align_score (where = 1)
on a state: upload, the state's buffers and stream."""
import ctypes as C
import os

import numpy as np
import pytest

import align_cases
import wsynth
from conftest import ROOT

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(ROOT, "tests", "native", "libalign_kernels.so")
CASES = align_cases.cases()


@pytest.fixture(scope="module")
def expected():
    """the float64 yardstick of every case, computed once"""
    return {name: align_cases.expected(logits, target) for name, logits, target in CASES}


@pytest.fixture(scope="module")
def har(wrs):
    assert os.path.exists(HARNESS), "tests/native/libalign_kernels.so missing: make -C whisper-rust_amd align_harness (__graft_entry__.build() does)"
    lib = C.CDLL(HARNESS)
    rec = C.POINTER(wrs.whisper_amd_align_score)
    lib.align_kernels_run.restype = C.c_int
    lib.align_kernels_run.argtypes = [C.POINTER(C.c_float), C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, rec]
    lib.align_kernels_host.restype = None
    lib.align_kernels_host.argtypes = [C.POINTER(C.c_float), C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_int32), rec]
    return lib


def run(har, wrs, logits, target, ld=None, off=0, host=False):
    n_rows, n_vocab = logits.shape
    ld = n_vocab if ld is None else ld
    buf = np.full((n_rows, ld), np.nan, np.float32)
    buf[:, :n_vocab] = logits
    tgt = np.ascontiguousarray(target, np.int32)
    out = (wrs.whisper_amd_align_score * n_rows)()
    a = (buf.ctypes.data_as(C.POINTER(C.c_float)), ld, n_rows, n_vocab, tgt.ctypes.data_as(C.POINTER(C.c_int32)))
    if host:
        har.align_kernels_host(*a, out)
    else:
        assert har.align_kernels_run(*a, off, out) == 0
    return np.frombuffer(out, dtype=wrs.ALIGN_SCORE_DTYPE).copy()


def check(got, want, host, name):
    for r, (g, w, h) in enumerate(zip(got, want, host)):
        plog, p, best, best_plog, best_p, rank = w
        d = [align_cases.ulps32(g["plog"], plog), align_cases.ulps32(g["p"], p), align_cases.ulps32(g["best_plog"], best_plog),
             align_cases.ulps32(g["best_p"], best_p)]
        print("%s row %d: ulps plog %d p %d best_plog %d best_p %d; best_id %d / %d, rank %d / %d" % (name, r, *d, g["best_id"], best, g["rank"], rank))
        assert g["best_id"] == best == h["best_id"] and g["rank"] == rank == h["rank"], (name, r)
        assert max(d) <= 1, (name, r, d)


@pytest.mark.parametrize("n_vocab", align_cases.N_VOCABS)
def test_kernel_scores_against_float64(har, wrs, expected, n_vocab):
    mine = [c for c in CASES if c[1].shape[1] == n_vocab]
    assert mine
    for name, logits, target in mine:
        got = run(har, wrs, logits, target)
        check(got, expected[name], run(har, wrs, logits, target, host=True), name)
        assert run(har, wrs, logits, target).tobytes() == got.tobytes(), name           # two device runs: the same bits


@pytest.mark.parametrize("n_vocab", [5, 257, 51865])
def test_rows_off_the_16_byte_boundary(har, wrs, expected, n_vocab):
    """3 rows at ld = n_vocab (odd: the rows lie 0, 4, 8 bytes ... off a boundary in turn), at ld = n_vocab + 3, and with the first row 1..3
    floats off: the same records as on the boundary, to the ulp bound, and the same best_id and rank"""
    name, logits, target = next(c for c in CASES if c[1].shape == (3, n_vocab))
    host = run(har, wrs, logits, target, host=True)
    for ld, off in [(n_vocab, 0), (n_vocab + 3, 0), (n_vocab, 1), (n_vocab, 2), (n_vocab + 3, 3), (n_vocab + 1, 1)]:
        got = run(har, wrs, logits, target, ld=ld, off=off)
        check(got, expected[name], host, "%s ld %d off %d" % (name, ld, off))
        assert run(har, wrs, logits, target, ld=ld, off=off).tobytes() == got.tobytes()


def test_through_the_state(wrs, amd_lib, expected):
    """whisper_amd_align_score: where = 1 is the product launcher on the state's stream, where = 0 the host function; refused arguments write nothing"""
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    st = ctx.create_state()
    for name, logits, target in [c for c in CASES if c[1].shape[1] in (257, 51865) and c[1].shape[0] == 3][:4]:
        dev, host = st.align_score(logits, target, where=1), st.align_score(logits, target, where=0)
        check(dev, expected[name], host, name)
        check(host, expected[name], host, name)
        assert st.align_score(logits, target, where=1).tobytes() == dev.tobytes()
    rows = st.align_stats()[1]
    assert rows > 0 and st.align_stats()[0] == 0 and st.align_stats()[2] == 0       # rows scored by the kernel; no align() call was made
    _, logits, target = CASES[0]
    for bad in ([logits.shape[1]], [-1]):
        with pytest.raises(wrs.WhisperError) as e:
            st.align_score(logits[:1], bad, where=1)
        assert e.value.code == wrs.ALIGN_NO_TOKENS
    with pytest.raises(wrs.WhisperError):
        st.align_score(logits[:1], target[:1], where=2)
    assert st.align_stats()[1] == rows
    st.free()
    ctx.free()

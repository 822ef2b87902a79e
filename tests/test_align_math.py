"""The alignment scores, host part (whisper-rust_amd/csrc/wa_align.h behind tests/native/align_math.cpp, compiled alone by g++: no HIP, no device).

The yardstick is numpy float64 with math.fsum for the sum (tools/align_cases.py).  n_vocab in {1, 3, 4, 5, 255, 256, 257, 1023, 51865, 51866},
1..3 rows, rows that are random N(0, 3), all equal, tied for the maximum at two indices, with the target the best or the last index, with one
logit 1e4 above the rest, with -inf logits and with a -inf target.

best_id and rank are exact.  plog, best_plog and p lie within 1 ulp (F32) of the float64 value rounded to F32.  That bound is derived, not
measured: an F64 sum of at most 51866 non-negative terms, an F64 exp and an F64 log are each accurate to about 1e-15 relative, eight orders
below half an F32 ulp, so the one rounding that matters is the final conversion to F32 - and one more ulp is granted for the case where the
F64 value lies so close to the middle between two F32 values that its last bits decide the direction.  CPU only."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import align_cases
import whisper_rs as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "align_math.cpp")
INC = "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc")
CASES = align_cases.cases()


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("align_math") / "libalign_math.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", INC, "-shared", "-o", so, SRC, "-lm"])
    lib = C.CDLL(so)
    lib.align_math_score.restype = None
    lib.align_math_score.argtypes = [C.POINTER(C.c_float), C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_int32), C.POINTER(W.whisper_amd_align_score)]
    lib.align_math_sizes.restype = C.c_int
    lib.align_math_sizes.argtypes = [C.c_int]
    return lib


def score(drv, logits, target, ld=None):
    n_rows, n_vocab = logits.shape
    if ld is None:
        ld = n_vocab
    buf = np.full((n_rows, ld), np.nan, np.float32)
    buf[:, :n_vocab] = logits
    tgt = np.ascontiguousarray(target, np.int32)
    out = (W.whisper_amd_align_score * n_rows)()
    drv.align_math_score(buf.ctypes.data_as(C.POINTER(C.c_float)), ld, n_rows, n_vocab, tgt.ctypes.data_as(C.POINTER(C.c_int32)), out)
    return np.frombuffer(out, dtype=W.ALIGN_SCORE_DTYPE).copy()


def check(got, want, name):
    """`want` from align_cases.expected; prints every figure before it asserts"""
    for r, (g, w) in enumerate(zip(got, want)):
        plog, p, best, best_plog, best_p, rank = w
        d = [align_cases.ulps32(g["plog"], plog), align_cases.ulps32(g["p"], p), align_cases.ulps32(g["best_plog"], best_plog),
             align_cases.ulps32(g["best_p"], best_p)]
        print("%s row %d: ulps plog %d p %d best_plog %d best_p %d; best_id %d / %d, rank %d / %d" % (name, r, *d, g["best_id"], best, g["rank"], rank))
        assert g["best_id"] == best and g["rank"] == rank, (name, r)
        assert max(d) <= 1, (name, r, d)


def test_layout_is_the_headers(drv):
    assert drv.align_math_sizes(0) == 24 == C.sizeof(W.whisper_amd_align_score) == W.ALIGN_SCORE_DTYPE.itemsize
    assert drv.align_math_sizes(1) == 32 == C.sizeof(W.whisper_amd_align_token)


def test_the_cases_hold_what_they_claim():
    names = [c[0] for c in CASES]
    for n in align_cases.N_VOCABS:
        for kind in align_cases.KINDS:
            assert any(s.startswith("v%d_" % n) and s.endswith(kind) for s in names), (n, kind)
        assert {int(s.split("_")[1][1:]) for s in names if s.startswith("v%d_" % n)} == set(align_cases.N_ROWS)


@pytest.mark.parametrize("n_vocab", align_cases.N_VOCABS)
def test_host_scores_against_float64(drv, n_vocab):
    mine = [c for c in CASES if c[1].shape[1] == n_vocab]
    assert mine
    for name, logits, target in mine:
        check(score(drv, logits, target), align_cases.expected(logits, target), name)


def test_row_stride_wider_than_the_vocabulary(drv):
    name, logits, target = next(c for c in CASES if c[0].startswith("v257_r3_random"))
    assert (score(drv, logits, target, ld=260).tobytes() == score(drv, logits, target).tobytes())


def test_kernel_uses_no_scratch(tmp_path):
    """k_align_score compiled for gfx950 with the product's flags: the compiler's own resource remarks show no scratch and no spilled register"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-slp-vectorize",
                        "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(ROOT, "whisper-rust_amd", "csrc", "wa_align.hip"),
                        "-o", str(tmp_path / "wa_align_k.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stderr.splitlines()
    at = next(i for i, s in enumerate(lines) if "Function Name:" in s and "k_align_score" in s)
    seen = {}
    for s in lines[at + 1:]:
        if "Function Name:" in s:
            break
        for key in ("ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Dynamic Stack"):
            if "remark:" in s and key + ":" in s:
                seen[key] = s.split(key + ":")[1].split("[")[0].strip()
    print(seen)
    assert seen == {"ScratchSize [bytes/lane]": "0", "SGPRs Spill": "0", "VGPRs Spill": "0", "Dynamic Stack": "False"}, seen


def test_named_properties(drv):
    rng = np.random.default_rng(5)
    x = rng.normal(0, 3, (1, 1023)).astype(np.float32)
    # a tie for the maximum: the lowest index is the model's choice, the later one has rank 1
    x[0, 700] = x[0, 40] = np.float32(50.0)
    g = score(drv, x, [700])[0]
    assert g["best_id"] == 40 and g["rank"] == 1 and g["plog"] == g["best_plog"]
    assert score(drv, x, [40])[0]["rank"] == 0
    # one logit 1e4 above the rest: lse == mx, so the others' plog is x_t - mx exactly and their p is 0
    x[0, 40] = np.float32(1.0e4)
    g = score(drv, x, [3])[0]
    assert g["plog"] == np.float32(np.float64(x[0, 3]) - np.float64(x[0, 40])) and g["p"] == 0.0 and g["best_plog"] == 0.0 and g["best_p"] == 1.0
    # all equal: every index has p = 1 / n, and the rank is the index
    e = np.full((1, 256), np.float32(-2.5))
    g = score(drv, e, [255])[0]
    assert g["best_id"] == 0 and g["rank"] == 255 and g["p"] == np.float32(1.0 / 256) and g["plog"] == np.float32(-np.log(256.0))
    # a -inf target: plog -inf, p 0, behind every finite logit and the earlier -inf ones
    x = rng.normal(0, 3, (1, 5)).astype(np.float32)
    x[0, 1] = x[0, 3] = -np.inf
    g = score(drv, x, [3])[0]
    assert g["plog"] == -np.inf and g["p"] == 0.0 and g["rank"] == 4

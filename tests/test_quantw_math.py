"""The weight quantisers stated in host code (whisper-rust_amd/csrc/wa_quantw.h: wa_quantw_rows for Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q4_K,
Q5_K and Q6_K) must give the bytes of the reference library's own ggml_quantize_chunk, from F32 values and from F16 values widened
exactly, on one fixed set of rows that takes every branch of the block arithmetic (quantw_rows below).  CPU only."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")
SRC = os.path.join(ROOT, "tests", "native", "quantw_math.cpp")
INC = os.path.join(ROOT, "whisper-rust_amd", "csrc")
TYPES = {"q4_0": 2, "q4_1": 3, "q5_0": 6, "q5_1": 7, "q8_0": 8, "q4_k": 12, "q5_k": 13, "q6_k": 14}


def quantw_rows() -> np.ndarray:
    """The rows every quantw test uses, F32, 17 super-blocks of 256 values."""
    rng = np.random.default_rng(7)
    g = lambda n: rng.standard_normal(n, dtype=np.float32)
    zb = g(256); zb[64:96] = 0.0                                       # an all-zero block (and K sub-block)
    twice = 0.1 * g(256); twice[35] = 2.5; twice[49] = -2.5            # the largest magnitude twice, opposite signs: the first wins
    clamp = 0.2 * g(256); clamp[0] = -1.0; clamp[1] = 0.999            # 0.999 * 8 + 8.5 = 16.49 and 0.999 * 16 + 16.5 = 32.48: the clamps
    equal = g(256); equal[96:128] = 0.37                               # a K sub-block with max == min
    pos = g(256); pos[160:192] = np.abs(pos[160:192]) + 0.5            # all positive: min clamps to 0, this_min > 0 is taken
    sub = (rng.integers(-1023, 1024, 256) * 2.0 ** -24).astype(np.float32)      # F16 subnormals
    big = g(256); big *= np.float32(6e4) / np.abs(big).max()           # near the F16 limit
    return np.concatenate([g(256), g(768), g(1280), zb, np.zeros(256, np.float32), twice, clamp, equal, pos, sub, big])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    d = tmp_path_factory.mktemp("quantw")
    exe = str(d / "quantw_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-I", INC, "-o", exe, "-ldl"])
    rows = quantw_rows()
    rows.tofile(str(d / "rows.f32"))
    rows.astype(np.float16).tofile(str(d / "rows.f16"))
    return exe, str(d / "rows.f32"), str(d / "rows.f16"), rows.size // 256


@pytest.mark.parametrize("name", list(TYPES))
def test_quantw_rows_equal_reference(driver, name):
    exe, f32, f16, nsb = driver
    t = TYPES[name]
    out = subprocess.run([exe, REF_LIB, str(t), f32, f16], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    nblk = nsb * (8 if t < 12 else 1)
    for src in (0, 1):
        assert "quantw: type %d src %d blocks %d bad 0" % (t, src, nblk) in out.stdout
    assert "quantw: refusals 1 2 3" in out.stdout

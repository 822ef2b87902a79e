"""The Q4_0 and Q4_K arithmetic stated in host code (whisper-rust_amd/csrc/wa_quant4.h: block unpack, the interleaved kernel layouts, the Q8_0 row and
the Q8_K row of the four-row quantiser, one output of the interleaved products - Q4_0: ONE fma chain over the blocks; Q4_K: two, stepping per block or per
pair of sub-blocks by the row's place - and of the plain products, the embedding's dequantisation) must equal the reference library bit for bit.  The
library is asked through one-node MUL_MAT graphs whose weight lies in its CPU repack buffer type, so it chooses quantiser, interleave and gemv / gemm
itself: M in {1, 3, 4, 5, 7, 8, 21}, K in {32, 96, 768} (Q4_K: {256, 768}), N = 16; and with N = 9 rows in its plain buffer (ggml_vec_dot_q4_0_q8_0 /
q4_K_q8_K, dequantize_row_q4_0 / q4_K).  Q4_K rows hold - m before + m once below M - M % 4 and once as a leftover row.  tests/native/quant4_math.cpp.
CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")
SRC = os.path.join(ROOT, "tests", "native", "quant4_math.cpp")
INC = os.path.join(ROOT, "whisper-rust_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_q4_arithmetic_equals_reference(tmp_path, flags):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    exe = str(tmp_path / "quant4_math")
    # no -mfma and contraction off: a * b + c in the header is two roundings, fmaf one, as in the library's build
    subprocess.check_call(["g++", *flags, "-std=c++17", "-ffp-contract=off", SRC, "-I", INC, "-o", exe, "-ldl"])
    out = subprocess.run([exe, REF_LIB], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2500:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "quant4: 0 mismatches" in out.stdout, out.stdout[-4000:]

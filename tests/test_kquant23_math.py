"""The Q2_K / Q3_K block arithmetic stated in host code (whisper-rust_amd/csrc/wa_quantk.h: the loader's block unpack, the token
embedding's dequantisation and one output of either product on a Q8_K activation row) must equal the reference library's own
dequantize_row_q2_K / q3_K and ggml_vec_dot_q2_K_q8_K / q3_K_q8_K bit for bit: rows quantised by quantize_row_q2_K_ref / q3_K_ref and rows
of raw random block bytes (d / dmin of both signs, tiny and zero), K = 256, 512, 768, 1024 and 5120, activation rows on the Q8_K rounding
points (tests/native/kquant23_math.cpp).  A Q3_K row, unpacked, is a Q6_K row: the Q6_K product of the same arrays is held to
ggml_vec_dot_q3_K_q8_K too.  Deliberately wrong variants - Q2_K: the minimum term after the product term, the minimums as a scalar chain
added after hsum, either fma as a multiplication and an addition, swapped scale / minimum nibbles; Q3_K: an inverted high bit, the upper
scale bits from the wrong byte; both: another hsum order - must each change some expected value.  The Q2_K kernels are a code object of
their own (wa_quantk_q2.o); none of them may spill or touch scratch.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")
SRC = os.path.join(ROOT, "tests", "native", "kquant23_math.cpp")
INC = os.path.join(ROOT, "whisper-rust_amd", "csrc")
VARIANTS = ("Q2_K minimum term after the product term", "Q2_K minimums as a scalar chain", "Q2_K minimum term not fused", "Q2_K product term not fused",
            "Q2_K swapped scale nibbles", "Q3_K inverted high bit", "Q3_K upper scale bits of the wrong byte", "Q2_K other hsum order", "Q3_K other hsum order")


def _run(exe):
    out = subprocess.run([exe, REF_LIB], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2500:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "kquant23: 0 mismatches" in out.stdout, out.stdout[-4000:]
    for v in VARIANTS:
        line = [l for l in out.stdout.splitlines() if l.startswith("kquant23: variant %s changes " % v)]
        assert line and int(line[0].split()[-2]) > 0, (v, line)


def test_q2_K_q3_K_block_arithmetic_equals_reference(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    exe = str(tmp_path / "kquant23_math")
    # no -mfma and contraction off: a * b + c in the header is two roundings, fmaf one, as in the library's build
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-I", INC, "-o", exe, "-ldl"])
    _run(exe)


def test_q2_K_q3_K_block_arithmetic_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (host code only): every index of the two
    unpacks and of the products stays inside its array, no shift or conversion is undefined."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    exe = str(tmp_path / "kquant23_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC,
                           "-I", INC, "-o", exe, "-ldl"])
    _run(exe)


def test_q2_K_kernels_use_no_scratch(tmp_path):
    """The Q2_K instantiations - 7 epilogues x (8-row, one-row), the only kernels of wa_quantk_q2.o - have no scratch and no spilled
    register.  Read from the code object the build just made."""
    tools = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(ROOT, "whisper-rust_amd", "build", "wa_quantk_q2.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(tools, "clang-offload-bundler")):
        pytest.skip("no build tree / LLVM tools here")
    fat, co = str(tmp_path / "fat"), str(tmp_path / "co")
    subprocess.check_call([os.path.join(tools, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(tools, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    notes = subprocess.check_output([os.path.join(tools, "llvm-readelf"), "--notes", co], text=True)
    seen, name = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith(".name:"):
            name = line.split(":", 1)[1].strip()
        elif name and (line.startswith(".private_segment_fixed_size:") or line.startswith(".vgpr_spill_count:") or line.startswith(".sgpr_spill_count:")):
            seen.setdefault(name, {})[line.split(":")[0]] = int(line.split(":")[1])
    assert len([k for k in seen if "k_kgemm_exact" in k]) == 7 and len([k for k in seen if "k_kgemv_exact" in k]) == 7 and len(seen) == 14, sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

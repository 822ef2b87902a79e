"""The Q5_K / Q6_K block arithmetic stated in host code (whisper-rust_amd/csrc/wa_quantk.h: the loader's block unpack, the token
embedding's dequantisation, the Q8_K quantisation of an activation row with its 16-element sums, and one output of either product, Q5_K
with its scalar chain over the sub-block minimums) must equal the reference library's own quantize_row_q8_K, dequantize_row_q5_K / q6_K
and ggml_vec_dot_q5_K_q8_K / q6_K_q8_K bit for bit: rows of K = 256, 512, 768, 1024, 3072 and 5120 and rows built to sit on the rounding
points (tests/native/kquant_math.cpp).  Deliberately wrong variants - a last-index maximum, a non-fused lane chain, another hsum order,
swapped nibble halves, either other rounding of the summs step - must each change some expected value.  The GPU kernels of
wa_quantk.hip restate this header; none of them may spill or touch scratch.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")
SRC = os.path.join(ROOT, "tests", "native", "kquant_math.cpp")
INC = os.path.join(ROOT, "whisper-rust_amd", "csrc")
VARIANTS = ("last-index maximum", "swapped nibble halves", "non-fused chain", "other hsum order", "summs as one fma", "summs added early")


def _run(exe):
    out = subprocess.run([exe, REF_LIB], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2500:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-4000:]
    assert "kquant: 0 mismatches" in out.stdout, out.stdout[-4000:]
    for v in VARIANTS:
        line = [l for l in out.stdout.splitlines() if l.startswith("kquant: variant %s changes " % v)]
        assert line and int(line[0].split()[-2]) > 0, (v, line)


def test_q5_K_q6_K_block_arithmetic_equals_reference(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    exe = str(tmp_path / "kquant_math")
    # no -mfma and contraction off: a * b + c in the header is two roundings, fmaf one, as in the library's build
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-I", INC, "-o", exe, "-ldl"])
    _run(exe)


def test_block_arithmetic_under_sanitizers(tmp_path):
    """The same stand-alone program built with AddressSanitizer and UndefinedBehaviorSanitizer (host code only): every index of the unpack,
    the layout map and the products stays inside its array, no shift or conversion is undefined."""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    exe = str(tmp_path / "kquant_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC,
                           "-I", INC, "-o", exe, "-ldl"])
    _run(exe)


def test_kquant_kernels_use_no_scratch(tmp_path):
    """Every kernel of wa_quantk.hip - the quantiser, the embedding, 7 epilogues x (8-row, one-row) x (Q5_K, Q6_K) - has no scratch and no
    spilled register.  Read from the code object the build just made."""
    tools = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(ROOT, "whisper-rust_amd", "build", "wa_quantk.o")
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
    assert len([k for k in seen if "k_kgemm_exact" in k]) == 14 and len([k for k in seen if "k_kgemv_exact" in k]) == 14, sorted(seen)
    assert any("k_quantize_q8_K" in k for k in seen) and any("k_dec_embed_k" in k for k in seen), sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

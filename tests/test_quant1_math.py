"""The Q4_1 / Q5_1 block arithmetic stated in host code (whisper-rust_amd/csrc/wa_quant1.h: the loader's block unpack, the token
embedding's dequantisation, the Q8_1 quantisation of an activation row with its block sums, and one output of the product with its
second, scalar chain over the block minimums) must equal the reference library's own quantize_row_q8_1, dequantize_row_q4_1 / q5_1 and
ggml_vec_dot_q4_1_q8_1 / q5_1_q8_1 bit for bit: rows of K = 128, 384, 768, 3072 and rows built to sit on the rounding points.  The GPU
kernels of wa_quant.hip restate this function.  CPU only."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")


def test_q4_1_q5_1_block_arithmetic_equals_reference(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    if not os.path.exists(REF_LIB):
        pytest.skip("reference library not built")
    exe = str(tmp_path / "quant1_math")
    # no -mfma and contraction off: a * b + c in the header is two roundings, fmaf one, as in the library's build
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "native", "quant1_math.cpp"),
                           "-I", os.path.join(ROOT, "whisper-rust_amd", "csrc"), "-o", exe, "-ldl"])
    out = subprocess.run([exe, REF_LIB], capture_output=True, text=True, timeout=600)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert "quant1: 0 mismatches" in out.stdout, out.stdout[-4000:]


def test_q1_product_kernels_use_no_scratch(tmp_path):
    """The Q4_1 / Q5_1 instantiations of the quantised products (wa_quant.hip: k_qgemm_exact<.., true>, k_qgemv_exact<.., true>,
    k_qgemv_gelu_q8<true>) carry a second set of prefetch registers for the minimums and block sums: none of them may spill or touch
    scratch memory (a reload waits behind the lane's outstanding weight loads).  Read from the code object the build just made."""
    tools = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(ROOT, "whisper-rust_amd", "build", "wa_quant.o")
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
    q1 = [k for k in seen if "Lb1E" in k and ("k_qgemm_exact" in k or "k_qgemv_exact" in k or "k_qgemv_gelu_q8" in k)]
    assert len(q1) == 15, sorted(seen)          # 7 epilogues x (8-row, one-row) + the fused GELU product
    for k in q1:
        assert seen[k] == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, seen[k])

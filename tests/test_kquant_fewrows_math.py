"""The code object of the K formats' few-rows kernel (whisper-rust_amd/csrc/wa_quantk_rows.hip -> build/wa_quantk_rows.o): it exists wherever the
product was built, holds exactly the 5 epilogues (the decoder's) x 3 formats (Q6_K with Q3_K, Q5_K, Q2_K) x 7 row counts (2 .. 8) instantiations
of k_kgemv_rows and nothing else - the general kernels stay in wa_quantk.o / wa_quantk_q2.o, whose kernel counts tests/test_kquant_math.py and
tests/test_kquant23_math.py pin - and none of them has scratch or a spilled register.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "whisper-rust_amd", "build")
TOOLS = "/opt/rocm/lib/llvm/bin"
EPILOGUES, FORMATS, ROW_COUNTS = 5, 3, 7          # no class was taken out of the code


def test_kgemv_rows_instantiations_use_no_scratch(tmp_path):
    """Read from the code object the build just made, as tests/test_kquant_mfma_math.py reads wa_quantk_mfma.o."""
    if not os.path.exists(os.path.join(BUILD, "wa_quantk.o")):
        pytest.skip("no build tree here")
    obj = os.path.join(BUILD, "wa_quantk_rows.o")
    assert os.path.exists(obj), "the build made wa_quantk.o but not wa_quantk_rows.o"
    fat, co = str(tmp_path / "fat"), str(tmp_path / "co")
    subprocess.check_call([os.path.join(TOOLS, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(TOOLS, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    notes = subprocess.check_output([os.path.join(TOOLS, "llvm-readelf"), "--notes", co], text=True)
    seen, name = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith(".name:"):
            name = line.split(":", 1)[1].strip()
        elif name and (line.startswith(".private_segment_fixed_size:") or line.startswith(".vgpr_spill_count:") or line.startswith(".sgpr_spill_count:")):
            seen.setdefault(name, {})[line.split(":")[0]] = int(line.split(":")[1])
    count = EPILOGUES * FORMATS * ROW_COUNTS
    assert count == 105
    assert len([k for k in seen if "k_kgemv_rows" in k]) == count and len(seen) == count, sorted(seen)
    assert not [k for k in seen if "k_kgemm_exact" in k or "k_kgemv_exact" in k], sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

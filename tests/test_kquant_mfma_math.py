"""The code object of the K formats' matrix-core kernel (whisper-rust_amd/csrc/wa_quantk_mfma.hip -> build/wa_quantk_mfma.o): it exists wherever the
product was built, holds exactly the 7 epilogues x 3 formats (Q6_K with Q3_K, Q5_K, Q2_K) x 2 forms (four rows per lane, one row per lane)
instantiations of k_kgemm_mfma and nothing else, and none of them has scratch or a spilled register.  CPU only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "whisper-rust_amd", "build")
TOOLS = "/opt/rocm/lib/llvm/bin"


def test_kgemm_mfma_instantiations_use_no_scratch(tmp_path):
    """Read from the code object the build just made, as tests/test_kquant_math.py reads wa_quantk.o."""
    if not os.path.exists(os.path.join(BUILD, "wa_quantk.o")):
        pytest.skip("no build tree here")
    obj = os.path.join(BUILD, "wa_quantk_mfma.o")
    assert os.path.exists(obj), "the build made wa_quantk.o but not wa_quantk_mfma.o"
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
    assert len([k for k in seen if "k_kgemm_mfma" in k]) == 7 * 3 * 2 and len(seen) == 7 * 3 * 2, sorted(seen)
    assert not [k for k in seen if "k_kgemm_exact" in k or "k_kgemv_exact" in k], sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

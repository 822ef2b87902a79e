"""The few-rows product kernel of wa_quant.hip, what the CPU can say of it: every instantiation of k_qgemv_rows - 5 decoder epilogues x
(without, with a minimum) x R = 2..8 activation rows - is in the code object the build made, and none of them has scratch or a spilled
register (R accumulators beside four prefetched load groups: the register count is the kernel's risk).  The kernel itself runs in
tests/test_quant_fewrows_gpu.py."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_few_rows_kernels_use_no_scratch(tmp_path):
    """Read from the notes of build/wa_quant.o."""
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
    rows = {k: v for k, v in seen.items() if "k_qgemv_rows" in k}
    assert len(rows) == 5 * 2 * 7, sorted(rows)
    for k, v in rows.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

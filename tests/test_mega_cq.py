"""The ggml-small-width one-launch kernel (k_decode_mega_cq: the cross-attention role computes its own query, wa_mega.hip) keeps the
rule of the other persistent decode kernels: no scratch memory and no spilled VGPRs (a reload waits behind the wave's outstanding
weight loads).  Read from the code objects the build made; no GPU needed."""
import os
import subprocess

import pytest

from conftest import ROOT


def _kernel_notes(obj, tmp_path):
    tools = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(obj) or not os.path.exists(os.path.join(tools, "clang-offload-bundler")):
        pytest.skip("no build tree / LLVM tools here")
    fat, co = str(tmp_path / "fat"), str(tmp_path / "co")
    subprocess.check_call([os.path.join(tools, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(tools, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co])
    notes = subprocess.check_output([os.path.join(tools, "llvm-readelf"), "--notes", co], text=True)
    seen, name = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith(".name:"):
            name = line.split(":", 1)[1].strip()
        elif name and (line.startswith(".private_segment_fixed_size:") or line.startswith(".vgpr_spill_count:")):
            seen.setdefault(name, {})[line.split(":")[0]] = int(line.split(":")[1])
    return seen


@pytest.mark.parametrize("obj", ["wa_mega_cq.o", "wa_mega_cq_chaos.o"])
def test_own_query_kernel_uses_no_scratch(obj, tmp_path):
    seen = _kernel_notes(os.path.join(ROOT, "whisper-rust_amd", "build", obj), tmp_path)
    kernels = [k for k in seen if k.startswith("_Z16k_decode_mega_cq")]
    assert len(kernels) == 1, sorted(seen)
    assert seen[kernels[0]] == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0}, seen[kernels[0]]

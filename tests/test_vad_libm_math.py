"""wa_libm.h (whisper-rust_amd/csrc): the tanhf and expf that k_vad_lstm runs on the device, compiled by g++ alone and held to THIS process's
libm bit for bit (tests/native/vad_libm_math.cpp; at most 16 threads).  tanhf: every positive F32 from 2^-60 to 23, negatives at stride 61;
expf: every F32 of [-104, 89] from 2^-30 up in magnitude, stride 61 below; +-0, +-inf, NaN, the largest and smallest subnormals; and the
probe set of the load-time guard holds every branch edge +-1 ulp with both signs.  CPU only."""
import os
import subprocess

import pytest
from conftest import ROOT


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vad_libm") / "vad_libm_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-pthread",
                           os.path.join(ROOT, "tests", "native", "vad_libm_math.cpp"), "-o", exe, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    return {f[0]: f[1:] for f in (line.split() for line in out.stdout.splitlines())}


@pytest.mark.parametrize("name,at_least", [("tanhf_pos", 540000000), ("tanhf_neg", 8800000), ("tanhf_special", 14), ("expf_pos", 305000000),
                                           ("expf_neg", 307000000), ("expf_pos_small", 13000000), ("expf_neg_small", 13000000), ("expf_special", 14),
                                           ("edges", 21), ("guard", 65536)])       # edges lacking in the guard's probe set; the guard's verdict here
def test_bit_exact_against_libm(sweeps, name, at_least):
    n, bad, first = sweeps[name]
    assert int(n) >= at_least and int(bad) == 0, "%s: %s of %s arguments differ, first at bits 0x%s" % (name, bad, n, first)

"""Quantising a model file on the device, on the s256 synthetic model (d = 256: the smallest shape all eight types accept).
whisper_amd_quantize_file must write the file the reference's quantize tool writes (wsynth.quant_model_path), byte for byte;
whisper_amd_init_from_file_quantized on the F16 file must leave the weight arena, whisper_model_ftype and one greedy full() of loading that
file - Q4_0 / Q4_K in a fresh process with WHISPER_AMD_REPACK_ORDER=1, the host path in one with WHISPER_AMD_LOAD_HOST=1.  Q2_K, an input
that is already quantised and a d = 384 model with a K type are refused with an error."""
import os
import subprocess
import sys

import pytest

import wsynth
from test_quantw_math import TYPES

pytestmark = pytest.mark.gpu
PLAIN = [n for n in TYPES if n not in ("q4_0", "q4_k")]      # loadable without the switch
CHILD = """
import sys
sys.path[:0] = [%r, %r]
import wsynth, whisper_rs as W
lib = W.load_library()
a = W.WhisperContext.new_quantized(wsynth.model_path("s256"), %d, lib=lib)
b = W.WhisperContext.new_with_params(wsynth.quant_model_path("s256", %r), lib=lib)
assert (a.arena() == b.arena()).all() and a.model_ftype() == b.model_ftype()
print("same arena", a.load_stats()["path"], a.load_stats()["kernels"] > b.load_stats()["kernels"])
"""


def test_quantize_file_equals_reference_tool(wrs, amd_lib, tmp_path):
    for name, t in TYPES.items():
        out = str(tmp_path / (name + ".bin"))
        assert amd_lib.whisper_amd_quantize_file(wsynth.model_path("s256").encode(), out.encode(), t) == 0, name
        assert open(out, "rb").read() == open(wsynth.quant_model_path("s256", name), "rb").read(), name


@pytest.fixture(scope="module")
def pcm():
    return wsynth.synth_audio(480000, 0)


@pytest.mark.parametrize("name", PLAIN)
def test_quantize_at_load_equals_the_quantised_file(wrs, amd_lib, pcm, name):
    a = wrs.WhisperContext.new_quantized(wsynth.model_path("s256"), TYPES[name], lib=amd_lib)
    b = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s256", name), lib=amd_lib)
    assert (a.arena() == b.arena()).all() and a.model_ftype() == b.model_ftype()
    sa, sb = a.load_stats(), b.load_stats()
    assert sa["path"] == 1 and sa["bytes_read"] == sb["bytes_read"] and sa["kernels"] > sb["kernels"]
    segs = []
    for ctx in (a, b):
        st = ctx.create_state()
        st.full(wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0), pcm)
        segs.append(st.segments())
        st.free(); ctx.free()
    assert segs[0] and segs[0] == segs[1]


@pytest.mark.parametrize("name,env,says", [("q4_0", "WHISPER_AMD_REPACK_ORDER", "same arena 1 True"), ("q4_k", "WHISPER_AMD_REPACK_ORDER", "same arena 1 True"),
                                           ("q5_0", "WHISPER_AMD_LOAD_HOST", "same arena 0 False"), ("q6_k", "WHISPER_AMD_LOAD_HOST", "same arena 0 False")])
def test_quantize_at_load_in_a_fresh_process(name, env, says):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = CHILD % (os.path.join(root, "whisper-rust_amd"), os.path.join(root, "tools"), TYPES[name], name)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{env: "1"}), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and says in out.stdout, out.stdout[-1500:] + out.stderr[-1500:]


def test_refusals(wrs, amd_lib, tmp_path):
    errors = []
    wrs.set_log_callback(amd_lib, lambda lvl, txt: errors.append(txt) if lvl == 4 else None)
    out = str(tmp_path / "no.bin")
    try:
        for src, t, word in ((wsynth.model_path("s256"), 10, "Q2_K"), (wsynth.quant_model_path("s256", "q5_0"), 8, "already quantised"),
                             (wsynth.model_path("tiny"), 13, "multiple")):
            del errors[:]
            assert amd_lib.whisper_amd_quantize_file(src.encode(), out.encode(), t) == wrs.QUANTIZE_REFUSED and not os.path.exists(out)
            assert any(word in e for e in errors), errors
            del errors[:]
            with pytest.raises(wrs.WhisperError):
                wrs.WhisperContext.new_quantized(src, t, lib=amd_lib)
            assert any(word in e for e in errors), errors
    finally:
        wrs.set_log_callback(amd_lib, None)

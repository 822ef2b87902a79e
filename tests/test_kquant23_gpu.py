"""Q2_K / Q3_K model files (MI355X): the two remaining K formats the reference multiplies in plain row order, through the K-format x Q8_K
products of wa_quantk.hip (the arithmetic: whisper-rust_amd/csrc/wa_quantk.h, held to the reference library on the CPU by
tests/test_kquant23_math.py; the kernels one by one: tests/test_kquant23_kernels_gpu.py).

  * goldens from the reference engine on s256 (tests/golden/s256_kquant23.json, tools/gen_golden_kquant23.py): encoder digest,
    teacher-forced logits digests, greedy, the default ladder, beam 3, the streaming call pattern; greedy and beam 3 again on the stalled
    test build;
  * the reference engine itself (oracle/_ref/libwhisper_ref.so) run LIVE beside the product on base:q2_k and base:q3_k (d = 512, two blocks
    per row, the smallest real shape): encoder output, prompt / single-token / 5-token logits, a greedy full();
  * the model's ftype, both one-launch forms off, every environment switch against the default path, a lock-step group against its members
    alone, and the load errors (a width that holds no 256-value block, a truncated file).
Everything is equality of bytes or of token lists.  Before these formats loaded, every test here that opens a q2_k / q3_k file failed with
"unsupported ftype 10" / "unsupported ftype 11"."""
import ctypes as C
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import wsynth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAOS_LIB = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")
FTYPE = {"q2_k": 10, "q3_k": 11}
QTYPES = pytest.mark.parametrize("qt", ["q2_k", "q3_k"])


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _segs(st):
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"], tids=s["tids"],
                 p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]]) for s in st.segments()]


def _get(lib, fn, st, n):
    f = getattr(lib, fn)
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64]
    out = np.empty(n, np.float32)
    r = f(st.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n)
    assert r == n, (fn, r, n)
    return out


def _params(wrs, lib, kw, **extra):
    kk = {k: v for k, v in kw.items() if k != "strategy"}
    kk.update(extra)
    return wrs.FullParams(lib, kw.get("strategy", 0), **kk)


@pytest.fixture(scope="module")
def gold():
    return json.load(open(os.path.join(GOLDEN, "s256_kquant23.json")))


def test_goldens_are_not_collapsed(gold):
    """Every recorded full() run holds at least 10 distinct token ids (the generator asserts the same)."""
    for qt, gd in gold.items():
        for tag, sg in gd["full"].items():
            assert len({i for s in sg for i in s["ids"]}) >= 10, (qt, tag)


@QTYPES
def test_q2_k_q3_k_models_bit_exact_against_goldens(wrs, amd_lib, gold, qt):
    """s256 quantised to Q2_K / Q3_K by the reference's own tool: encoder output and teacher-forced logits (a 3-token prompt, single steps, a
    5-token batch, 40 tokens) bit-identical to the reference engine (digests), identical segments / ids / p / plog for greedy, the temperature
    ladder and beam 3, and the streaming pattern."""
    import gen_golden_quant as g
    gd = gold[qt]
    mp = wsynth.quant_model_path("s256", qt)
    assert hashlib.sha256(open(mp, "rb").read()).hexdigest() == gd["model_sha256"], "the quantised model file differs from the goldens'"
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    d = ctx.model_n_audio_state()
    st = ctx.create_state()
    st.pcm_to_mel(wsynth.synth_audio(480000, 0)); st.encode(0)
    assert digest(_get(amd_lib, "whisper_amd_get_embd_enc", st, 1500 * d)) == gd["embd_enc"]["sha256"]
    for e in gd["logits"]:
        st.decode(e["tokens"], e["n_past"])
        lg = st.get_logits_last(len(e["tokens"]))
        assert digest(lg) == e["sha256"], "logits %r n_past %d: top %d vs %d" % (e["tokens"][:3], e["n_past"], int(np.argmax(lg)), e["top"])
    st.free()
    for tag, kw in g.FULL.items():
        for aseed in (0, 1):
            st = ctx.create_state()
            st.full(_params(wrs, amd_lib, kw), wsynth.synth_audio(480000, aseed))
            assert _segs(st) == gd["full"]["%s_seed%d" % (tag, aseed)], (qt, tag, aseed)
            st.free()
    assert g.stream_run(wrs, amd_lib, ctx) == gd["stream"]
    ctx.free()


@QTYPES
def test_q2_k_q3_k_models_on_the_stalled_build(wrs, gold, qt):
    """Greedy and beam 3 on the test build with stalled product waves: the goldens again (results must not depend on timing)."""
    import gen_golden_quant as g
    chaos = wrs.load_library(CHAOS_LIB)
    wrs.set_log_callback(chaos, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s256", qt), wrs.WhisperContextParameters(chaos), lib=chaos)
    for tag in ("greedy", "beam3"):
        st = ctx.create_state()
        st.full(_params(wrs, chaos, g.FULL[tag]), wsynth.synth_audio(480000, 0))
        assert _segs(st) == gold[qt]["full"]["%s_seed0" % tag], (qt, tag)
        st.free()
    ctx.free()


@pytest.mark.parametrize("name", ["base:q2_k", "base:q3_k"])
def test_base_live_beside_the_reference(wrs, amd_lib, ref_lib, name):
    """base (d = 512: two blocks per row, eight in the second MLP product): encoder output, the logits of a 3-token prompt, of a single token
    and of a 5-token batch, and a greedy full() equal to the reference engine's on the same file and inputs (whatever it returns: on this
    synthetic model and audio the reference's full() of base:q2_k ends without a segment; the s256 goldens are the full() runs with content)."""
    mp = wsynth.quant_model_path(*name.split(":"))
    a = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    r = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(ref_lib, use_gpu=False), lib=ref_lib)
    d = a.model_n_audio_state()
    ref_lib.ref_shim_get_embd_enc.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    pcm = wsynth.synth_audio(480000, 0)
    sa, sr = a.create_state(), r.create_state()
    sa.pcm_to_mel(pcm); sa.encode(0)
    sr.pcm_to_mel(pcm, 8); sr.encode(0, 16)
    x = np.empty(1500 * d, np.float32)
    ref_lib.ref_shim_get_embd_enc(sr.ptr, x.ctypes.data_as(C.POINTER(C.c_float)), x.size)
    assert digest(_get(amd_lib, "whisper_amd_get_embd_enc", sa, 1500 * d)) == digest(x), name
    sot = a.token_sot()
    for toks, n_past in (([sot, sot + 1, a.token_transcribe()], 0), ([a.token_beg() + 3], 3), ([4321, 777, 31000, 15, 50], 4)):
        sa.decode(toks, n_past); sr.decode(toks, n_past, 16)
        assert digest(sa.get_logits_last(len(toks))) == digest(sr.get_logits_last(len(toks))), (name, toks, n_past)
    sa.free(); sr.free()
    sa, sr = a.create_state(), r.create_state()
    kw = dict(best_of=1, temperature_inc=0.0)
    sa.full(wrs.FullParams(amd_lib, 0, **kw), pcm)
    sr.full(wrs.FullParams(ref_lib, 0, n_threads=16, **kw), pcm)
    got, want = _segs(sa), _segs(sr)
    assert got == want, name
    sa.free(); sr.free()
    a.free(); r.free()


def test_ftype_and_forms_off(wrs, amd_lib):
    """whisper_model_ftype names the format (10 Q2_K, 11 Q3_K); both one-launch forms are off for it (their kernels read Q5_0 / Q8_0 blocks of 32)
    and a beam run has not gone near the several-rows kernel."""
    amd_lib.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    amd_lib.whisper_amd_rows_enabled.argtypes = [C.c_void_p]
    for qt, ft in FTYPE.items():
        ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s256", qt), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
        assert ctx.model_ftype() == ft
        st = ctx.create_state()
        st.full(wrs.FullParams(amd_lib, 1, beam_size=3, temperature_inc=0.0), wsynth.synth_audio(480000, 3))
        assert amd_lib.whisper_amd_mega_enabled(st.ptr) == 0 and amd_lib.whisper_amd_rows_enabled(st.ptr) == 0, qt
        assert st.rows_stats() == (0, 0), (qt, st.rows_stats())
        st.free()
        ctx.free()


SWITCHES = [{"WHISPER_AMD_ROWS_HOST_OUT": "0"}, {"WHISPER_AMD_NO_RUN_AHEAD": "1"}, {"WHISPER_AMD_NO_ROWS": "1"}, {"WHISPER_AMD_NO_BATCHER": "1"},
            {"WHISPER_AMD_NO_MEGA": "1", "WHISPER_AMD_NO_ROWS": "1"}, {"WHISPER_AMD_NO_OVERLAP": "1"}, {"WHISPER_AMD_SINGLE_ROWS": "1"},
            {"WHISPER_AMD_SINGLE_ROWS": "0"}, {"WA_LIB": CHAOS_LIB}, {"WHISPER_AMD_ROWS_FORCE_INORDER": "1"}, {"WHISPER_AMD_NO_GRAPH": "1"},
            {"WHISPER_AMD_NO_EXACT_MFMA": "1"}]


def _switch_digest(env_extra):
    env = dict(os.environ); env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "switch_check.py"), "s256:q2_k"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env_extra, r.stdout[-400:], r.stderr[-800:])
    line = [l for l in r.stdout.splitlines() if l.startswith("digest")]
    assert line, (env_extra, r.stdout[-400:])
    assert int(line[-1].split()[-1]) > 0, line
    return line[-1]


@pytest.fixture(scope="module")
def default_digest():
    return _switch_digest({})


@pytest.mark.parametrize("env_extra", SWITCHES, ids=["+".join("%s=%s" % (k.replace("WHISPER_AMD_", ""), os.path.basename(v)) for k, v in e.items()) for e in SWITCHES])
def test_environment_switch_does_not_change_a_bit_q2_k(default_digest, env_extra):
    """Each of the backend's switches (read once per process: one fresh process each, tools/switch_check.py - four chunks in a lock-step group,
    greedy, beam 5, best_of 3 with the ladder) gives the default path's digest on s256:q2_k; the tests above hold the default path to the
    reference."""
    assert _switch_digest(env_extra) == default_digest, env_extra


def test_lockstep_group_of_q2_k_chunks_equals_solo(wrs, amd_lib):
    """Four s256:q2_k chunks through whisper_amd_full_batch: each chunk's segments equal its solo run's."""
    mp = wsynth.quant_model_path("s256", "q2_k")
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcms = [wsynth.synth_audio(480000, 50 + i) for i in range(4)]
    fp = wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0)
    solo = []
    for p in pcms:
        st = ctx.create_state(); st.full(fp, p); solo.append(_segs(st)); st.free()
    assert any(solo)
    states = [ctx.create_state() for _ in pcms]
    wrs.full_batch(ctx, states, fp, pcms)
    for i, st in enumerate(states):
        assert _segs(st) == solo[i], i
        st.free()
    ctx.free()


def _load_fails(wrs, amd_lib, path):
    log = []
    wrs.set_log_callback(amd_lib, lambda lvl, txt: log.append(txt))
    try:
        with pytest.raises(wrs.WhisperError):
            wrs.WhisperContext.new_with_params(path, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    finally:
        wrs.set_log_callback(amd_lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    return "".join(log)


def test_load_errors(wrs, amd_lib, tmp_path):
    """An ftype-10 header on a d = 384 model (its rows hold no 256-value block) and a truncated q3_k file each fail at load with a message
    that says why."""
    src = wsynth.model_path("tiny")
    raw = bytearray(open(src, "rb").read(4 + 11 * 4))
    assert struct.unpack_from("<i", raw, 4 + 2 * 4)[0] == 384
    struct.pack_into("<i", raw, 4 + 10 * 4, 10)
    bad = str(tmp_path / "tiny-ftype10.bin")
    with open(src, "rb") as f, open(bad, "wb") as o:
        f.seek(len(raw)); o.write(raw); o.write(f.read())
    text = _load_fails(wrs, amd_lib, bad)
    assert "multiple of 256" in text and "384" in text and "Q2_K" in text, text[-600:]

    full = open(wsynth.quant_model_path("s256", "q3_k"), "rb").read()
    cut = str(tmp_path / "s256-q3_k-cut.bin")
    open(cut, "wb").write(full[:len(full) - 100000])
    text = _load_fails(wrs, amd_lib, cut)
    assert "truncated tensor" in text or "not all tensors loaded" in text, text[-600:]

"""Q5_1 / Q4_1 model files (MI355X): the formats of the published quantised tiny / base / small models, through the Q4_1 / Q5_1 x Q8_1
products of wa_quant.hip (the arithmetic: whisper-rust_amd/csrc/wa_quant1.h, held to the reference library on the CPU by
tests/test_quant1_math.py).

  * goldens from the reference engine (tests/golden/s128_quant1.json, tools/gen_golden_quant1.py);
  * the reference engine itself (oracle/_ref/libwhisper_ref.so) run LIVE beside the product on the shapes of the three published files
    and on small:q4_1 (teacher-forced passes of 1, 3, 5 and 8 rows, greedy full()), on s192:q5_1 (a width whose block count is not a multiple
    of 4), and for several decoders (beam 5 / 8, best_of 5 with the ladder) on the product and on its stalled test build;
  * every environment switch against the default path, a lock-step group against its members alone, the model's ftype, and the clean
    refusal of a Q4_0 file.
Everything is equality of bytes or of token lists.  These models decode through the launch sequence: the one assertion on the form here is
that both one-launch forms are OFF for them (their kernels read Q5_0 / Q8_0 quants)."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wsynth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAOS_LIB = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")


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


def _both(wrs, amd_lib, ref_lib, mp):
    a = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    r = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(ref_lib, use_gpu=False), lib=ref_lib)
    return a, r


@pytest.mark.parametrize("qt", ["q5_1", "q4_1"])
def test_q1_models_bit_exact_against_goldens(wrs, amd_lib, qt):
    """s128 quantised to Q5_1 / Q4_1 by the reference's own tool: encoder output and teacher-forced logits bit-identical to the reference
    engine (digests), identical segments / ids / p / plog for greedy, the temperature ladder and beam search, and the streaming pattern."""
    import gen_golden_quant as g
    gold = json.load(open(os.path.join(GOLDEN, "s128_quant1.json")))[qt]
    mp = wsynth.quant_model_path("s128", qt)
    assert hashlib.sha256(open(mp, "rb").read()).hexdigest() == gold["model_sha256"], "the quantised model file differs from the goldens'"
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    d = ctx.model_n_audio_state()
    st = ctx.create_state()
    st.pcm_to_mel(wsynth.synth_audio(480000, 0)); st.encode(0)
    assert digest(_get(amd_lib, "whisper_amd_get_embd_enc", st, 1500 * d)) == gold["embd_enc"]["sha256"]
    for e in gold["logits"]:
        st.decode(e["tokens"], e["n_past"])
        lg = st.get_logits_last(len(e["tokens"]))
        assert digest(lg) == e["sha256"], "logits %r n_past %d: top %d vs %d" % (e["tokens"][:3], e["n_past"], int(np.argmax(lg)), e["top"])
    st.free()
    for tag, kw in g.FULL.items():
        for aseed in (0, 1):
            st = ctx.create_state()
            st.full(_params(wrs, amd_lib, kw), wsynth.synth_audio(480000, aseed))
            assert _segs(st) == gold["full"]["%s_seed%d" % (tag, aseed)], (qt, tag, aseed)
            st.free()
    got = g.stream_run(wrs, amd_lib, ctx)
    assert got == gold["stream"]
    ctx.free()


@pytest.mark.parametrize("name", ["tiny:q5_1", "base:q5_1", "small:q5_1", "small:q4_1", "s192:q5_1"])
def test_published_shapes_live_beside_the_reference(wrs, amd_lib, ref_lib, name):
    """The shapes of ggml-tiny-q5_1 / ggml-base-q5_1 / ggml-small-q5_1 (and small as Q4_1): encoder output, the logits of a 3-token prompt,
    of a single token, of a 5-token batch, of 8 decoder rows (a full tile of the several-rows product: every lane's minimum chain is handed
    over) and of 5 rows again behind them, and a greedy full() - ids / p / plog / segments - equal to the reference engine's on the same file
    and inputs.  s192 (d = 192: 6 blocks per row, not a multiple of 4) takes the products' block-by-block loops, which no published width does."""
    mp = wsynth.quant_model_path(*name.split(":"))
    a, r = _both(wrs, amd_lib, ref_lib, mp)
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
    for toks, n_past in (([sot, sot + 1, a.token_transcribe()], 0), ([a.token_beg() + 3], 3), ([4321, 777, 31000, 15, 50], 4),
                          ([220, 1000, 50, 2425, 11, 257, 40000, 13], 9), ([3, 99, 25000, 764, 1], 17)):
        sa.decode(toks, n_past); sr.decode(toks, n_past, 16)
        assert digest(sa.get_logits_last(len(toks))) == digest(sr.get_logits_last(len(toks))), (name, toks, n_past)
    fkw = dict(strategy=0, best_of=1, temperature_inc=0.0, language="en", no_context=True)
    sa.full(_params(wrs, amd_lib, fkw), pcm)
    sr.full(_params(wrs, ref_lib, fkw, n_threads=16), pcm)
    info_r, info_g = (C.c_double * 8)(), (C.c_double * 8)()
    ids_r, ids_g = (C.c_int32 * 512)(), (C.c_int32 * 512)()
    ref_lib.ref_shim_decoder_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int]
    amd_lib.whisper_amd_decoder_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int]
    n_r = ref_lib.ref_shim_decoder_info(sr.ptr, 0, info_r, ids_r, 512)
    n_g = amd_lib.whisper_amd_decoder_info(sa.ptr, 0, info_g, ids_g, 512)
    assert n_r > 0 and n_r == n_g and list(ids_r[:n_r]) == list(ids_g[:n_g]), name
    assert list(info_r) == list(info_g), name
    assert _segs(sa) == _segs(sr), name
    for x_ in (sa, sr):
        x_.free()
    a.free(); r.free()


@pytest.mark.parametrize("name", ["s128:q5_1", "small:q5_1", "tiny:q5_1", "small:q4_1"])
def test_several_decoders_live_and_under_stalls(wrs, amd_lib, ref_lib, name):
    """Beam 5, beam 8 and best_of 5 on the temperature ladder: segments identical to the reference engine's run in the same test, on the
    product and on its test build with stalled waves (results must not depend on timing)."""
    mp = wsynth.quant_model_path(*name.split(":"))
    chaos = wrs.load_library(CHAOS_LIB)
    wrs.set_log_callback(chaos, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    r = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(ref_lib, use_gpu=False), lib=ref_lib)
    pcm = wsynth.synth_audio(480000, 2)
    modes = {"beam5": dict(strategy=1, beam_size=5, temperature_inc=0.0), "beam8": dict(strategy=1, beam_size=8, temperature_inc=0.0),
             "best_of5": dict(strategy=0, best_of=5, temperature=0.4, temperature_inc=0.2)}
    want = {}
    for tag, kw in modes.items():
        sr = r.create_state()
        sr.full(_params(wrs, ref_lib, kw, n_threads=16), pcm)
        want[tag] = _segs(sr)
        sr.free()
    r.free()
    assert any(len(v) > 0 for v in want.values())
    for lib in (amd_lib, chaos):
        a = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(lib), lib=lib)
        for tag, kw in modes.items():
            sa = a.create_state()
            sa.full(_params(wrs, lib, kw), pcm)
            assert _segs(sa) == want[tag], (name, tag, "stalled build" if lib is chaos else "product")
            sa.free()
        a.free()


def test_environment_switches_do_not_change_a_bit_q5_1():
    """Every combination of the backend's switches (read once per process: one fresh process each, tools/switch_check.py - four chunks in a
    lock-step group, greedy, beam 5, best_of 3 with the ladder) gives ONE digest on s128:q5_1; the tests above hold the default path to the
    reference."""
    combos = [{}, {"WHISPER_AMD_ROWS_HOST_OUT": "0"}, {"WHISPER_AMD_NO_RUN_AHEAD": "1"}, {"WHISPER_AMD_NO_ROWS": "1"}, {"WHISPER_AMD_NO_BATCHER": "1"},
              {"WHISPER_AMD_NO_MEGA": "1", "WHISPER_AMD_NO_ROWS": "1"}, {"WHISPER_AMD_NO_OVERLAP": "1"}, {"WHISPER_AMD_SINGLE_ROWS": "1"},
              {"WHISPER_AMD_SINGLE_ROWS": "0"}, {"WA_LIB": CHAOS_LIB}, {"WHISPER_AMD_ROWS_FORCE_INORDER": "1"},
              {"WHISPER_AMD_ROWS_FORCE_INORDER": "1", "WA_LIB": CHAOS_LIB}]
    lines = []
    for env_extra in combos:
        env = dict(os.environ); env.update(env_extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "switch_check.py"), "s128:q5_1"], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (env_extra, r.stdout[-400:], r.stderr[-800:])
        line = [l for l in r.stdout.splitlines() if l.startswith("digest")]
        assert line, (env_extra, r.stdout[-400:])
        lines.append(line[-1])
    assert len(set(lines)) == 1, list(zip([str(c) for c in combos], lines))


def test_lockstep_group_of_q5_1_chunks_equals_solo(wrs, amd_lib):
    """Four small:q5_1 chunks through whisper_amd_full_batch: each chunk's segments equal its solo run's."""
    mp = wsynth.quant_model_path("small", "q5_1")
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcms = [wsynth.synth_audio(480000, 50 + i) for i in range(4)]
    fp = wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0)
    solo = []
    for p in pcms:
        st = ctx.create_state(); st.full(fp, p); solo.append(_segs(st)); st.free()
    states = [ctx.create_state() for _ in pcms]
    wrs.full_batch(ctx, states, fp, pcms)
    for i, st in enumerate(states):
        assert _segs(st) == solo[i], i
        st.free()
    ctx.free()


def test_ftype_and_refusal_of_q4_0(wrs, amd_lib):
    """whisper_model_ftype names the format (9 Q5_1, 3 Q4_1) and both one-launch forms are off for it; a Q4_0 file, written by the same tool, is refused at load with the list of
    supported formats in the log (the reference multiplies Q4_0 in a repacked form whose order is not restated here)."""
    amd_lib.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    amd_lib.whisper_amd_rows_enabled.argtypes = [C.c_void_p]
    for qt, ft in (("q5_1", 9), ("q4_1", 3)):
        ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s128", qt), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
        assert ctx.model_ftype() == ft
        # no one-launch kernel exists for these formats (k_decode_mega_q / k_decode_rows_q_np* read the quants as signed Q5_0 / Q8_0 values):
        # both forms must be off, and a beam run must not have gone near the several-rows kernel
        st = ctx.create_state()
        st.full(wrs.FullParams(amd_lib, 1, beam_size=5, temperature_inc=0.0), wsynth.synth_audio(480000, 3))
        assert amd_lib.whisper_amd_mega_enabled(st.ptr) == 0 and amd_lib.whisper_amd_rows_enabled(st.ptr) == 0, qt
        assert st.rows_stats() == (0, 0), (qt, st.rows_stats())
        st.free()
        ctx.free()
    log = []
    wrs.set_log_callback(amd_lib, lambda lvl, txt: log.append(txt))
    try:
        with pytest.raises(wrs.WhisperError):
            wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s128", "q4_0"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    finally:
        wrs.set_log_callback(amd_lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    text = "".join(log)
    assert "unsupported ftype 2" in text and all(n in text for n in ("F16", "Q8_0", "Q5_0", "Q5_1", "Q4_1")), text[-600:]

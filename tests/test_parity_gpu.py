"""Parity tests proper (MI355X): the product, called through its C ABI, against
  (1) the golden vectors the reference engine produced (tests/golden/, bit-exact digests and full segment lists),
  (2) the CPU oracle restatement run live at a mid size (tiny-shaped model),
  (3) size-independent properties at the BASELINE.json size (ggml-small shape).

Tolerances:
  flash_attn = false (default, reference summation order): BIT-EXACT - SHA-256 of the float bytes, identical token
      ids / timestamps / text / p / plog for greedy, temperature ladder (sampled) and beam search.
  flash_attn = true (MFMA path, different F32 summation order, same rounding points): mel bit-exact;
      |d embd_enc| <= 1e-2 (values in +-5); |d logits| <= 1e-3 * max|logit| (north_star's 1e-3 at unit logit scale);
      identical greedy token ids on the pinned cases.
"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import wsynth
from conftest import GOLDEN, ORACLE_LIB

pytestmark = pytest.mark.gpu


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _get(lib, fn, st, n):
    f = getattr(lib, fn)
    f.restype = C.c_int64
    f.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64]
    out = np.empty(n, np.float32)
    r = f(st.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n)
    assert r == n, (fn, r, n)
    return out


def _get_mel(lib, st):
    lib.whisper_amd_get_mel.restype = C.c_int64
    lib.whisper_amd_get_mel.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    nl, nm = C.c_int(), C.c_int()
    n = lib.whisper_amd_get_mel(st.ptr, None, 0, nl, nm)
    out = np.empty(n, np.float32)
    lib.whisper_amd_get_mel(st.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n, nl, nm)
    return out, nl.value, nm.value


def _segs(st):
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"], tids=s["tids"],
                 p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]]) for s in st.segments()]


def _same(a, b, exact_probs=True):
    assert len(a) == len(b), (len(a), len(b))
    for x, y in zip(a, b):
        assert (x["t0"], x["t1"], x["ids"], x["text"]) == (y["t0"], y["t1"], y["ids"], y["text"])
        if exact_probs:     # reference-order path: also the per-token probabilities and the argmax-timestamp ids, bit for bit
            assert x["tids"] == y["tids"] and x["p"] == y["p"] and x["plog"] == y["plog"]


@pytest.fixture(scope="module", params=["s128", "s192"])
def env(request, wrs, amd_lib):
    shape = request.param
    gold = json.load(open(os.path.join(GOLDEN, shape + ".json")))
    mp = wsynth.model_path(shape, gold["model_seed"])
    assert hashlib.sha256(open(mp, "rb").read()).hexdigest() == gold["model_sha256"]
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    yield dict(shape=shape, gold=gold, ctx=ctx, lib=amd_lib, wrs=wrs, mp=mp)
    ctx.free()


# ------------------------------------------------------------------------------------------------------------
# reference-order path: bit-exact against the reference engine's goldens
# ------------------------------------------------------------------------------------------------------------
def test_mel_bit_exact_all_lengths(env):
    for tag, g in env["gold"]["mel"].items():
        st = env["ctx"].create_state()
        st.pcm_to_mel(wsynth.synth_audio(g["n_samples"], g["audio_seed"]))
        mel, n_len, n_mel = _get_mel(env["lib"], st)
        assert (n_len, n_mel, st.n_len()) == (g["n_len"], 80, g["n_len_org"]), tag
        assert digest(mel) == g["sha256"], "mel " + tag
        st.free()


def test_encoder_and_logits_bit_exact(env):
    gold, lib, ctx = env["gold"], env["lib"], env["ctx"]
    d, nv = ctx.model_n_audio_state(), ctx.n_vocab()
    st = ctx.create_state()
    st.pcm_to_mel(wsynth.synth_audio(480000, 0))
    st.encode(0)
    assert digest(_get(lib, "whisper_amd_get_embd_conv", st, 1500 * d)) == gold["embd_conv"]["sha256"]
    assert digest(_get(lib, "whisper_amd_get_embd_enc", st, 1500 * d)) == gold["embd_enc"]["sha256"]
    for g in gold["logits"]:            # single tokens (GEMV path), 3/5-token batches, 40-token prompt (GEMM path)
        st.decode(g["tokens"], g["n_past"])
        lg = st.get_logits_last(len(g["tokens"]))
        assert lg.shape == (nv,)
        assert digest(lg) == g["sha256"], "logits %r" % (g["tokens"][:4],)
    st.encode(1000)
    assert digest(_get(lib, "whisper_amd_get_embd_enc", st, 1500 * d)) == gold["embd_enc_offset1000"]["sha256"]
    lang_id, probs = st.lang_detect(0)
    assert lang_id == gold["lang_detect"]["lang_id"] and digest(probs) == gold["lang_detect"]["probs_sha256"]
    st.free()


def _full_case_params(wrs, lib, kw):
    kk = {k: v for k, v in kw.items() if k != "strategy"}
    return wrs.FullParams(lib, kw.get("strategy", 0), **kk)


def test_full_transcription_matches_reference_in_every_mode(env):
    """greedy, temperature ladder (sampling), beam search, no_timestamps, single_segment+max_tokens, audio_ctx,
    offset/duration, prompt tokens with context, suppress_nst+translate: identical segments, ids, p, plog."""
    import gen_golden_cases as cases
    for tag, kw in cases.FULL_CASES.items():
        for aseed in (0, 1):
            st = env["ctx"].create_state()      # fresh state, as in the generator
            st.full(_full_case_params(env["wrs"], env["lib"], kw), wsynth.synth_audio(480000, aseed))
            try:
                _same(_segs(st), env["gold"]["full"]["%s_seed%d" % (tag, aseed)])
            except AssertionError as e:
                raise AssertionError("%s seed %d: %s" % (tag, aseed, e))
            st.free()


def test_dtw_token_timestamps_match_reference(env):
    """DTW token timestamps (BASELINE config 4): extra decoder pass capturing the alignment heads' cross-attention, then
    normalise / median / mean / DTW on the host - every t_dtw identical to the reference engine's."""
    import gen_golden_cases as cases
    wrs, lib = env["wrs"], env["lib"]
    for tag, preset, kw in cases.DTW_CASES:
        ctx = wrs.WhisperContext.new_with_params(env["mp"], wrs.WhisperContextParameters(lib, dtw_preset=preset, **kw), lib=lib)
        for aseed in (0, 1):
            st = ctx.create_state()
            st.full(wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0), wsynth.synth_audio(480000, aseed))
            got = [dict(t0=s["t0"], t1=s["t1"], ids=s["ids"], t_dtw=s["t_dtw"]) for s in st.segments()]
            assert got == env["gold"]["dtw"]["%s_seed%d" % (tag, aseed)], (tag, aseed)
            st.free()
        ctx.free()


def test_state_carried_across_calls_and_short_inputs(env):
    wrs, lib, ctx, gold = env["wrs"], env["lib"], env["ctx"], env["gold"]
    st = ctx.create_state()
    fp = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0, no_context=False)
    st.full(fp, wsynth.synth_audio(480000, 0)); a = _segs(st)
    st.full(fp, wsynth.synth_audio(480000, 1)); b = _segs(st)
    _same(a, gold["full"]["two_calls_same_state"][0]); _same(b, gold["full"]["two_calls_same_state"][1])
    st.free()
    for tag, n in (("1s", 16000), ("0.05s", 800)):      # 0.05 s: "input is too short" -> 0 segments, rc 0
        st = ctx.create_state()
        st.full(wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0), wsynth.synth_audio(n, 7))
        _same(_segs(st), gold["full"]["short_" + tag])
        st.free()
    st = ctx.create_state()
    with pytest.raises(wrs.WhisperError):                # whisper-rs: empty input is an error before the C call
        st.full(wrs.FullParams(lib, 0), np.zeros(0, np.float32))
    st.free()


def test_callbacks_and_device_resident_pcm(env):
    """new_segment / progress / encoder_begin / abort callbacks fire as in the reference; a HIP device pointer is
    accepted in place of host samples and gives the same result."""
    wrs, lib, ctx, gold = env["wrs"], env["lib"], env["ctx"], env["gold"]
    seen = dict(new=0, prog=[], enc=0)
    st = ctx.create_state()
    fp = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    fp.set("new_segment_callback", lambda c, s, n, u: seen.__setitem__("new", seen["new"] + n))
    fp.set("progress_callback", lambda c, s, p, u: seen["prog"].append(p))
    fp.set("encoder_begin_callback", lambda c, s, u: (seen.__setitem__("enc", seen["enc"] + 1), True)[1])
    pcm = wsynth.synth_audio(480000, 0)
    hip = C.CDLL("libamdhip64.so")
    dptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(dptr), C.c_size_t(pcm.nbytes)) == 0
    assert hip.hipMemcpy(dptr, C.c_void_p(pcm.ctypes.data), C.c_size_t(pcm.nbytes), 1) == 0
    st.full(fp, (dptr.value, len(pcm)))
    want = gold["full"]["greedy_tinc0_seed0"]
    _same(_segs(st), want)
    assert seen["new"] == len(want) and seen["enc"] >= 1 and seen["prog"] and seen["prog"][0] == 0
    hip.hipFree(dptr)
    # abort: the callback is polled after each pass; returning true fails the call with -6 (encode) like the reference
    st2 = ctx.create_state()
    fp2 = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    fp2.set("abort_callback", lambda u: True)
    with pytest.raises(wrs.WhisperError) as ei:
        st2.full(fp2, pcm)
    assert ei.value.code == -6
    st.free(); st2.free()


# ------------------------------------------------------------------------------------------------------------
# MFMA path (flash_attn = true): tolerance-level parity
# ------------------------------------------------------------------------------------------------------------
def test_flash_path_within_tolerance(env):
    wrs, lib, gold = env["wrs"], env["lib"], env["gold"]
    samples = np.load(os.path.join(GOLDEN, env["shape"] + "_samples.npz"))
    ctx = wrs.WhisperContext.new_with_params(env["mp"], wrs.WhisperContextParameters(lib, flash_attn=True), lib=lib)
    d = ctx.model_n_audio_state()
    st = ctx.create_state()
    st.pcm_to_mel(wsynth.synth_audio(480000, 0))
    mel, n_len, _ = _get_mel(lib, st)
    assert digest(mel) == gold["mel"]["30s_seed0"]["sha256"]                   # the mel kernel is shared: bit-exact
    st.encode(0)
    enc = _get(lib, "whisper_amd_get_embd_enc", st, 1500 * d).reshape(1500, d)[::25]
    assert np.abs(enc - samples["embd_enc"]).max() <= 1e-2
    for g in gold["logits"]:
        st.decode(g["tokens"], g["n_past"])
        lg = st.get_logits_last(len(g["tokens"]))
        ref = samples["logits_%d_%d" % (len(g["tokens"]), g["n_past"])]
        assert np.abs(lg - ref).max() <= 1e-3 * g["absmax"], (np.abs(lg - ref).max(), g["absmax"])
        assert int(lg.argmax()) == g["top_ids"][0]
    st.free()
    st = ctx.create_state()
    st.full(wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0), wsynth.synth_audio(480000, 0))
    segs, ref_segs = _segs(st), gold["full"]["greedy_tinc0_seed0"]
    st.free()
    a = [t for s in ref_segs for t in s["ids"]]
    b = [t for s in segs for t in s["ids"]]
    first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), None)
    if first is None:
        _same(segs, ref_segs, exact_probs=False)        # identical greedy token ids
    else:
        # The contract of this path is a tolerance, so a different token is legitimate exactly at a near tie: there the two runs pick
        # the two members of a top pair whose probabilities differ by less than the tolerance moves them (each run reports the
        # probability of the token it picked; away from a tie the winner's probability would be far above the runner-up's).
        pa = [x for s_ in ref_segs for x in s_["p"]]
        pb = [x for s_ in segs for x in s_["p"]]
        assert abs(pa[first] - pb[first]) <= 2e-2 * max(pa[first], pb[first]), (first, a[first], b[first], pa[first], pb[first])
        assert first >= 32, first                       # and not systematically: a long common prefix precedes it
    ctx.free()


def test_flash_path_small_audio_ctx(wrs, amd_lib):
    """The tolerance path on reduced audio contexts (streaming windows; a single key tile, tiles with few valid keys): finite and
    within the path's tolerance of the reference-order path, which the tests above pin to the reference."""
    amd_lib.whisper_amd_get_embd_enc.restype = C.c_int64
    amd_lib.whisper_amd_get_embd_enc.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64]
    pcm = wsynth.synth_audio(16000 * 2, 0)
    for actx in (50, 257):
        out = {}
        for flash in (False, True):
            ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=flash), lib=amd_lib)
            d = ctx.model_n_audio_state()
            st = ctx.create_state()
            st.full(wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0, audio_ctx=actx, single_segment=True), pcm)
            buf = np.zeros(1500 * d, np.float32)
            amd_lib.whisper_amd_get_embd_enc(st.ptr, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size)
            out[flash] = buf[:actx * d].copy()
            st.free(); ctx.free()
        assert np.isfinite(out[True]).all()
        assert np.abs(out[True] - out[False]).max() <= 1e-2, actx


@pytest.mark.parametrize("shape", ["tiny", "base", "small", "m1024", "w1280"])
def test_flash_path_at_model_widths(wrs, amd_lib, shape):
    """The tolerance path against the reference-order path of the same library at the real models' widths (d = 384, 512, 768, 1024,
    1280): encoder output at audio_ctx 1500 and 257 within 1e-2, and the logits after a 40-token prompt - the decoder's DEC_QKV /
    GELU_F16 / RESID products on the MFMA GEMM - within 1e-3 max|logit| with the same argmax.  The reference-order path is pinned to
    the reference at tiny, small and m1024 by the tests above; at base and w1280 this bounds the gap between the two paths only."""
    amd_lib.whisper_amd_get_embd_enc.restype = C.c_int64
    amd_lib.whisper_amd_get_embd_enc.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64]
    mp = wsynth.model_path(shape)
    toks = [50258, 50259, 50359, 50364] + list(range(300, 336))
    out = {}
    for flash in (False, True):
        ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib, flash_attn=flash), lib=amd_lib)
        d = ctx.model_n_audio_state()
        st = ctx.create_state()
        st.pcm_to_mel(wsynth.synth_audio(480000, 0))
        st.encode(0)
        enc = _get(amd_lib, "whisper_amd_get_embd_enc", st, 1500 * d)
        st.decode(toks, 0)
        lg = st.get_logits_last(len(toks))
        st.free()
        st = ctx.create_state()
        st.full(wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0, audio_ctx=257, single_segment=True), wsynth.synth_audio(32000, 0))
        buf = np.zeros(1500 * d, np.float32)
        amd_lib.whisper_amd_get_embd_enc(st.ptr, buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size)
        out[flash] = (enc, lg, buf[:257 * d].copy())
        st.free(); ctx.free()
    (e0, l0, s0), (e1, l1, s1) = out[False], out[True]
    de, ds, dl = np.abs(e1 - e0), np.abs(s1 - s0), np.abs(l1 - l0)
    print("\nflash vs exact %-6s d %4d: embd_enc max %.2e rms %.2e | audio_ctx 257 max %.2e rms %.2e | logits max %.2e (%.2e of max|logit| %.1f)"
          % (shape, d, de.max(), np.sqrt((de ** 2).mean()), ds.max(), np.sqrt((ds ** 2).mean()), dl.max(), dl.max() / np.abs(l0).max(),
             np.abs(l0).max()))
    assert np.isfinite(e1).all() and np.isfinite(s1).all() and np.isfinite(l1).all()
    assert de.max() <= 1e-2 and ds.max() <= 1e-2
    assert dl.max() <= 1e-3 * np.abs(l0).max()
    assert int(l1.argmax()) == int(l0.argmax())


# ------------------------------------------------------------------------------------------------------------
# mid size, live oracle; full size, properties
# ------------------------------------------------------------------------------------------------------------
def test_tiny_shape_bit_exact_against_live_oracle(wrs, amd_lib):
    """ggml-tiny shape (d = 384, 4+4 layers): encoder output and logits bit-identical to the CPU oracle run here."""
    assert os.path.exists(ORACLE_LIB), "oracle/liboracle.so missing"
    orc = C.CDLL(ORACLE_LIB)
    orc.wo_load.restype = C.c_void_p; orc.wo_load.argtypes = [C.c_char_p]; orc.wo_free.argtypes = [C.c_void_p]
    for f in ("wo_embd_enc", "wo_logits"):
        getattr(orc, f).restype = C.POINTER(C.c_float); getattr(orc, f).argtypes = [C.c_void_p]
    orc.wo_mel.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]; orc.wo_encode.argtypes = [C.c_void_p, C.c_int]
    orc.wo_decode.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.c_int]
    mp = wsynth.model_path("tiny")
    pcm = wsynth.synth_audio(480000, 3)
    m = orc.wo_load(mp.encode())
    orc.wo_mel(m, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm)); orc.wo_encode(m, 0)
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    st = ctx.create_state()
    st.pcm_to_mel(pcm); st.encode(0)
    d, nv = 384, ctx.n_vocab()
    assert digest(_get(amd_lib, "whisper_amd_get_embd_enc", st, 1500 * d)) == digest(np.ctypeslib.as_array(orc.wo_embd_enc(m), shape=(1500 * d,)))
    for toks, n_past in (([50258, 50259, 50359], 0), ([50364], 3), ([400, 500, 600], 4), ([11], 7)):
        arr = (C.c_int32 * len(toks))(*toks)
        orc.wo_decode(m, arr, len(toks), n_past)
        st.decode(toks, n_past)
        assert digest(st.get_logits_last(len(toks))) == digest(np.ctypeslib.as_array(orc.wo_logits(m), shape=(nv,)))
    orc.wo_free(m); st.free(); ctx.free()


def test_small_shape_properties(wrs, amd_lib):
    """BASELINE.json size (ggml-small shape).  The oracle needs minutes here, so: determinism (encode twice -> same
    digest), batch/sequential consistency (a 12-token prompt through the GEMM path == the same tokens fed one by one
    through the GEMV path, bit for bit), and KV re-decode idempotence (re-decoding from an earlier n_past reproduces
    the logits)."""
    mp = wsynth.model_path("small")
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    st = ctx.create_state()
    st.pcm_to_mel(wsynth.synth_audio(480000, 0))
    st.encode(0); e1 = digest(_get(amd_lib, "whisper_amd_get_embd_enc", st, 1500 * 768))
    st.encode(0); e2 = digest(_get(amd_lib, "whisper_amd_get_embd_enc", st, 1500 * 768))
    assert e1 == e2
    toks = [50258, 50259, 50359, 50364] + list(range(300, 308))
    st.decode(toks, 0); batch = st.get_logits_last(len(toks)).copy()
    for i, t in enumerate(toks):
        st.decode([t], i)
    seq = st.get_logits_last(1).copy()
    assert digest(batch) == digest(seq)
    st.decode(toks[8:], 8)
    assert digest(st.get_logits_last(len(toks) - 8)) == digest(batch)
    assert np.isfinite(batch).all()
    st.free(); ctx.free()


@pytest.mark.parametrize("name,n_tok", [("s128", 40), ("tiny", 24), ("base", 24), ("small", 48), ("m1024", 12), ("w1280", 12),
                                        ("s128:q5_0", 40), ("s128:q8_0", 40), ("small:q5_0", 40), ("w1280:q5_0", 12)])
def test_one_launch_decode_step_equals_launch_sequence(wrs, amd_lib, name, n_tok, monkeypatch):
    """The single-token decoder pass as ONE persistent launch (wa_mega.hip) against the launch sequence (which the tests
    above pin to the reference): bit-identical logits token by token, over enough tokens that n_kv crosses the n % 8 and
    n % 32 boundaries of the soft-max / P V leftovers; and the one-launch path must actually be the one that ran."""
    amd_lib.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    mp = wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)      # "small:q5_0" = the quantised file
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "1"); ref = ctx.create_state()
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "0"); meg = ctx.create_state()
    assert amd_lib.whisper_amd_mega_enabled(ref.ptr) == 0 and amd_lib.whisper_amd_mega_enabled(meg.ptr) == 1
    pcm = wsynth.synth_audio(480000, 1)
    sot = ctx.token_sot()
    prompt = [sot, sot + 1, sot + 102]
    for st in (ref, meg):
        st.pcm_to_mel(pcm); st.encode(0); st.decode(prompt, 0)
    tok = int(np.argmax(ref.get_logits_last(len(prompt))[:50000]))
    for i in range(n_tok):
        ref.decode([tok], len(prompt) + i); meg.decode([tok], len(prompt) + i)
        a = ref.get_logits_last(1); b = meg.get_logits_last(1)
        assert digest(a) == digest(b), "token %d (n_kv %d): max|d| = %g" % (i, len(prompt) + i + 1, float(np.abs(a - b).max()))
        tok = int(np.argmax(a[:50000]))
    assert amd_lib.whisper_amd_mega_enabled(meg.ptr) == 1, "the one-launch step gave up (hand-off time-out) and fell back"
    ref.free(); meg.free(); ctx.free()


@pytest.mark.parametrize("name,n_tok", [("small", 16), ("m1024", 12), ("w1280", 8), ("small:q5_0", 16), ("w1280:q5_0", 8), ("s128:q8_0", 12)])
def test_one_launch_step_under_stalls(wrs, name, n_tok, monkeypatch):
    """The same comparison on the test build whose product waves stall at random for ~25 us (libwhisper_chaos.so: wa_mega.hip with
    -DWA_CHAOS): the rest of the workgroup and of the grid then runs far ahead of the stalled wave, so anything in LDS that relied on
    how long a product or a hand-off takes shows up as different logits.  (The kernel as it was before the LayerNorm outputs got an
    LDS area of their own fails this on every token.)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(path)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    lib.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    mp = wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(lib), lib=lib)
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "1"); ref = ctx.create_state()
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "0"); meg = ctx.create_state()
    if lib.whisper_amd_mega_enabled(meg.ptr) != 1:
        pytest.skip("one-launch step switched off (WHISPER_AMD_NO_MEGA)")
    pcm = wsynth.synth_audio(480000, 2)
    sot = ctx.token_sot()
    prompt = [sot, sot + 1, sot + 102]
    for st in (ref, meg):
        st.pcm_to_mel(pcm); st.encode(0); st.decode(prompt, 0)
    tok = int(np.argmax(ref.get_logits_last(len(prompt))[:50000]))
    for i in range(n_tok):
        ref.decode([tok], len(prompt) + i); meg.decode([tok], len(prompt) + i)
        a = ref.get_logits_last(1); b = meg.get_logits_last(1)
        assert digest(a) == digest(b), "token %d: max|d| = %g" % (i, float(np.abs(a - b).max()))
        tok = int(np.argmax(a[:50000]))
    assert lib.whisper_amd_mega_enabled(meg.ptr) == 1, "the one-launch step gave up under the stalls"
    ref.free(); meg.free(); ctx.free()


@pytest.mark.parametrize("name", ["small", "m1024", "s128:q5_0"])
def test_several_rows_step_under_stalls(wrs, name, monkeypatch):
    """The several-rows one-launch step (wa_rows.hip) on the stalled test build (-DWA_CHAOS: waves and whole workgroups sleep ~25 us at random in
    front of products, attention units and gathers): batches of 2 / 5 / 8 tokens - causal masks, cells written by the launch itself - give the
    logits of the launch sequence, and every pass is served by the one-launch form."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(path)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    mp = wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(lib), lib=lib)
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "1"); ref = ctx.create_state()
    monkeypatch.setenv("WHISPER_AMD_NO_MEGA", "0"); row = ctx.create_state()
    if lib.whisper_amd_rows_enabled(row.ptr) != 1:
        pytest.skip("several-rows step not available")
    pcm = wsynth.synth_audio(480000, 2)
    for st in (ref, row):
        st.pcm_to_mel(pcm); st.encode(0)
    n_past = 0
    for rnd in range(3):
        for n in (3, 5, 8, 2):
            batch = [1000 + 37 * (n_past + i) for i in range(n)]
            ref.decode(batch, n_past); row.decode(batch, n_past)
            a = ref.get_logits_last(n); b = row.get_logits_last(n)
            assert digest(a) == digest(b), "batch of %d at n_past %d: max|d| = %g" % (n, n_past, float(np.abs(a - b).max()))
            n_past += n
    served, back = row.rows_stats()
    assert served == 12 and back == 0, (served, back)
    ref.free(); row.free(); ctx.free()


def test_lockstep_group_survives_a_failed_pass(wrs, amd_lib, monkeypatch):
    """A lock-step pass whose launch fails (forced through WHISPER_AMD_TEST_FAIL_BATCH_LAUNCH) must not hand out the stale contents of the
    staging buffer: every member then decodes alone, and each chunk's segments equal the goldens of the reference engine."""
    import json
    from conftest import GOLDEN
    import gen_golden_r2 as gen
    gold = json.load(open(os.path.join(GOLDEN, "r2_cases.json")))
    # (the hook is read once per process: the chunks run in a child process that starts with it set; this process never sees it)
    import subprocess
    code = ("import sys, json; sys.path[:0] = [%r, %r]; import wsynth, whisper_rs as W, gen_golden_r2 as gen\n"
            "lib = W.load_library(); W.set_log_callback(lib, None)\n"
            "ctx = W.WhisperContext.new_with_params(wsynth.model_path('s128'), W.WhisperContextParameters(lib), lib=lib)\n"
            "sts = [ctx.create_state() for _ in gen.BATCH_SEEDS]\n"
            "W.full_batch(ctx, sts, W.FullParams(lib, 0, best_of=1, temperature_inc=0.0), [wsynth.synth_audio(480000, s) for s in gen.BATCH_SEEDS])\n"
            "print(json.dumps([[dict(t0=s['t0'], t1=s['t1'], ids=s['ids']) for s in st.segments()] for st in sts]))\n"
            % (os.path.join(os.path.dirname(GOLDEN), "..", "tools"), os.path.join(os.path.dirname(GOLDEN), "..", "whisper-rust_amd")))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, timeout=600, env=dict(os.environ, WHISPER_AMD_TEST_FAIL_BATCH_LAUNCH="1"))
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-800:]
    got = json.loads(r.stdout.decode().strip().splitlines()[-1])
    for g, s in zip(got, gen.BATCH_SEEDS):
        want = [dict(t0=x["t0"], t1=x["t1"], ids=x["ids"]) for x in gold["s128"]["batch"]["seed%d" % s]]
        assert g == want, s


def test_full_transcription_under_stalls(wrs, monkeypatch):
    """whisper_full on the stalled test build: the greedy loop with the device predicting the next token (launches queued back to back,
    the host reading one launch's logits while the next runs) gives the segments of the launch sequence."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(path)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(lib), lib=lib)
    pcm = wsynth.synth_audio(480000, 3)
    fp = wrs.FullParams(lib, best_of=1, temperature_inc=0.0)
    out = {}
    for nomega in ("1", "0"):
        monkeypatch.setenv("WHISPER_AMD_NO_MEGA", nomega)
        st = ctx.create_state(); st.full(fp, pcm); out[nomega] = _segs(st); st.free()
    _same(out["1"], out["0"])
    assert sum(len(s_["ids"]) for s_ in out["1"]) > 0
    ctx.free()


def test_one_launch_step_reduced_audio_ctx(wrs, amd_lib, monkeypatch):
    """The one-launch step on reduced audio contexts (streaming windows): T below one 32-cell chain step, not a multiple of 8 / 32,
    a single leftover cell - segments, ids and probabilities identical to the launch sequence."""
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcm = wsynth.synth_audio(16000 * 3, 5)
    for actx in (1, 7, 33, 50, 257):
        res = {}
        for nomega in ("1", "0"):
            monkeypatch.setenv("WHISPER_AMD_NO_MEGA", nomega)
            st = ctx.create_state()
            st.full(wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0, audio_ctx=actx, single_segment=True), pcm)
            res[nomega] = [(s["t0"], s["t1"], s["ids"], s["p"], s["plog"]) for s in st.segments()]
            st.free()
        assert sum(len(s[2]) for s in res["0"]) > 0
        assert res["0"] == res["1"], actx
    ctx.free()


def test_host_overlap_never_changes_results(wrs, amd_lib, monkeypatch):
    """Greedy decoding with the device predicting the next token (host overlap) must give the segments of the plain loop -
    also when the prediction is wrong on purpose (every third token id hidden from the device), which exercises the
    discard-and-redo path; and the predictions must actually have been used / refused."""
    if os.environ.get("WHISPER_AMD_NO_MEGA", "0") not in ("", "0"):
        pytest.skip("the host overlap rides on the one-launch step, which WHISPER_AMD_NO_MEGA turns off")
    amd_lib.whisper_amd_overlap_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    amd_lib.whisper_amd_reset_timings.argtypes = [C.c_void_p]
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcm = wsynth.synth_audio(480000, 2)
    fp = wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0)
    out = {}
    for mode, env in (("plain", {"WHISPER_AMD_NO_OVERLAP": "1"}), ("overlap", {}), ("sabotage", {"WHISPER_AMD_OVERLAP_SABOTAGE": "1"})):
        for k in ("WHISPER_AMD_NO_OVERLAP", "WHISPER_AMD_OVERLAP_SABOTAGE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        st = ctx.create_state()
        amd_lib.whisper_amd_reset_timings(st.ptr)
        st.full(fp, pcm)
        ov = (C.c_int * 2)(); amd_lib.whisper_amd_overlap_stats(st.ptr, ov)
        out[mode] = (_segs(st), ov[0], ov[1])
        st.free()
    assert out["plain"][1] == 0 and out["plain"][2] == 0
    assert out["overlap"][1] > 0, "the overlap path did not run"
    assert out["sabotage"][2] > 0, "no wrong prediction was produced by the sabotaged mask"
    _same(out["plain"][0], out["overlap"][0]); _same(out["plain"][0], out["sabotage"][0])
    assert sum(len(s["ids"]) for s in out["plain"][0]) > 0
    ctx.free()


def test_heuristic_token_timestamps_and_segment_wrap_match_reference(wrs, amd_lib):
    """params.token_timestamps (+ max_len / split_on_word): per-token t0 / t1 / vlen from the |PCM| energy heuristic and the
    wrapped segments, identical to the reference engine's (goldens: tools/gen_golden_tts.py), with host and device PCM."""
    import ctypes as C2
    sys_path_tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    import sys
    if sys_path_tools not in sys.path:
        sys.path.insert(0, sys_path_tools)
    import gen_golden_tts as g
    gold = json.load(open(os.path.join(GOLDEN, "s128_token_ts.json")))
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    for tag, kw in g.TTS_CASES.items():
        for aseed in (0, 1):
            st = ctx.create_state()
            st.full(wrs.FullParams(amd_lib, 0, **kw), wsynth.synth_audio(480000, aseed))
            got, want = g.segs(st), gold["%s_seed%d" % (tag, aseed)]
            assert len(got) == len(want), (tag, aseed, len(got), len(want))
            for a, b in zip(got, want):
                assert a == b, (tag, aseed, a, b)
            st.free()
    ctx.free()


def test_full_parallel_is_the_concatenation_of_its_parts(wrs, amd_lib):
    """whisper_full_parallel (whisper.cpp:7736-7864) with n_processors = 2: the result on the context's own state equals
    transcribing the two halves separately, the second half shifted by the cut and clamped to start after the first ends."""
    lib = amd_lib
    mp = wsynth.model_path("s128").encode()
    cp = wrs.WhisperContextParameters(lib)
    lib.whisper_init_from_file_with_params.restype = C.c_void_p
    lib.whisper_init_from_file_with_params.argtypes = [C.c_char_p, type(cp.c)]
    fp = wrs.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    lib.whisper_full_parallel.restype = C.c_int
    lib.whisper_full_parallel.argtypes = [C.c_void_p, type(fp.c), C.POINTER(C.c_float), C.c_int, C.c_int]
    for f, rt in (("whisper_full_n_segments", C.c_int), ("whisper_full_get_segment_t0", C.c_int64), ("whisper_full_get_segment_t1", C.c_int64)):
        getattr(lib, f).restype = rt
    lib.whisper_full_n_segments.argtypes = [C.c_void_p]
    lib.whisper_full_get_segment_t0.argtypes = [C.c_void_p, C.c_int]; lib.whisper_full_get_segment_t1.argtypes = [C.c_void_p, C.c_int]
    lib.whisper_full_n_tokens.restype = C.c_int; lib.whisper_full_n_tokens.argtypes = [C.c_void_p, C.c_int]
    lib.whisper_full_get_token_id.restype = C.c_int; lib.whisper_full_get_token_id.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.whisper_free.argtypes = [C.c_void_p]
    pcm = wsynth.synth_audio(960000, 4)       # 60 s: two 30 s halves
    ctxp = lib.whisper_init_from_file_with_params(mp, cp.c)
    assert ctxp
    rc = lib.whisper_full_parallel(ctxp, fp.c, pcm.ctypes.data_as(C.POINTER(C.c_float)), len(pcm), 2)
    assert rc == 0
    got = [(lib.whisper_full_get_segment_t0(ctxp, i), lib.whisper_full_get_segment_t1(ctxp, i),
            [lib.whisper_full_get_token_id(ctxp, i, j) for j in range(lib.whisper_full_n_tokens(ctxp, i))]) for i in range(lib.whisper_full_n_segments(ctxp))]
    lib.whisper_free(ctxp)
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), cp, lib=lib)
    want = []
    half = len(pcm) // 2
    for k, part in enumerate((pcm[:half], pcm[half:])):
        st = ctx.create_state()
        st.full(fp, np.ascontiguousarray(part))
        for s in st.segments():
            t0, t1 = s["t0"] + k * (100 * half // 16000), s["t1"] + k * (100 * half // 16000)
            if want:
                t0 = max(t0, want[-1][1])
            want.append((t0, t1, s["ids"]))
        st.free()
    ctx.free()
    assert got == want and len(got) > 0


@pytest.mark.parametrize("qt", ["q5_0", "q8_0"])
def test_quantised_models_bit_exact(wrs, amd_lib, qt):
    """BASELINE config 5's weight format: a Q5_0 / Q8_0 model file (quantised by the reference's own tool) through the quantised
    products of wa_quant.hip - encoder output and teacher-forced logits bit-identical to the reference engine (digests), identical
    segments / ids / p / plog for greedy, the temperature ladder and beam search (goldens: tools/gen_golden_quant.py)."""
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_golden_quant as g
    gold = json.load(open(os.path.join(GOLDEN, "s128_quant.json")))[qt]
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
            kk = {k: v for k, v in kw.items() if k != "strategy"}
            st.full(wrs.FullParams(amd_lib, kw.get("strategy", 0), **kk), wsynth.synth_audio(480000, aseed))
            try:
                _same(_segs(st), gold["full"]["%s_seed%d" % (tag, aseed)])
            except AssertionError as ex:
                raise AssertionError("%s %s seed %d: %s" % (qt, tag, aseed, ex))
            st.free()
    # config 5's calling pattern: sliding windows with a reduced audio context, single segment, carried prompt tokens
    got = g.stream_run(wrs, amd_lib, ctx)
    assert len(got) == len(gold["stream"])
    for a, b in zip(got, gold["stream"]):
        _same(a, b)
    ctx.free()

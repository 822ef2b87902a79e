"""Forced alignment through the C ABI (whisper_amd_align, whisper-rust_amd/csrc/wa_align.cpp) on the synthetic models of tools/wsynth.py.

1. Times: on an s128 DTW context, for both presets of gen_golden_cases.DTW_CASES, full() (greedy, temperature_inc = 0) on 5 s of audio that it
   serves with ONE window - one encoder pass by the state's counter, and the window's frame count not cut short by a timestamp token - and then
   align() of the same audio with the text token ids of all segments: t_dtw equal, element for element, to what full() placed.
   tests/test_dtw_device_gpu.py holds full()'s t_dtw to the reference engine, so this ties align() to it with no new golden.  The same with
   WHISPER_AMD_DTW_HOST=1 in a child process.
2. Scores: for F16 s128, s128 Q5_0 and s256 Q6_K the logits of every scored row come from whisper_amd_decode_batch (eight flagged rows a
   pass, every pass the whole sequence: see logits_by_decode_batch); float64 log-softmax in numpy; plog, p and best_plog within 1 F32 ulp
   (the bound derived in tests/test_align_math.py), best_id and rank exact.
3. A better transcript scores better.  4. Refusals and hygiene.  5. The F16 scores once more on the build with stalled waves."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "whisper-rust_amd")):      # (the child process below runs this file as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import align_cases  # noqa: E402
import gen_golden_cases as cases  # noqa: E402
import wsynth  # noqa: E402

pytestmark = pytest.mark.gpu

N_SAMPLES = 80000          # 5 s: one window for both seeds below (found with the reference engine on the CPU)
SEEDS = (0, 2)             # seed 0: 147 text tokens and a closing timestamp beyond the audio; seed 2: 220 text tokens, no timestamp
MODELS = ["s128", "s128:q5_0", "s256:q6_k"]


def model_of(name):
    return wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)


def greedy(W, lib):
    return W.FullParams(lib, 0, best_of=1, temperature_inc=0.0)


def text_of(st, eot):
    """(ids, t_dtw) of the text tokens of all segments"""
    ids, t = [], []
    for s in st.segments():
        for i, d in zip(s["ids"], s["t_dtw"]):
            if i < eot:
                ids.append(i)
                t.append(d)
    return ids, t


def one_window_full(W, lib, ctx, pcm):
    """full() on a fresh state; asserts that it made exactly one window whose DTW frame count is the whole audio's"""
    st = ctx.create_state()
    st.full(greedy(W, lib), pcm)
    tm = (C.c_int64 * 12)()
    lib.whisper_amd_get_timings_us.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    lib.whisper_amd_get_timings_us(st.ptr, tm)
    assert tm[7] == 1, "full() encoded %d windows" % tm[7]
    info = (C.c_double * 8)()
    lib.whisper_amd_decoder_info.restype = C.c_int
    lib.whisper_amd_decoder_info.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int]
    lib.whisper_amd_decoder_info(st.ptr, 0, info, None, 0)
    assert info[3] >= st.n_len(), "the window's seek_delta %d cuts the DTW frames of %d" % (info[3], st.n_len())
    return st


def dtw_runs(W, lib):
    """{tag_seed: (ids, full()'s t_dtw, align()'s t_dtw, n segments)} and the DTW counters of the states, summed"""
    out, stats = {}, [0, 0, 0]
    for tag, preset, kw in cases.DTW_CASES:
        ctx = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(lib, dtw_preset=preset, **kw), lib=lib)
        for seed in SEEDS:
            pcm = wsynth.synth_audio(N_SAMPLES, seed)
            st = one_window_full(W, lib, ctx, pcm)
            ids, t_full = text_of(st, ctx.token_eot())
            n_seg = st.full_n_segments()
            st2 = ctx.create_state()
            al = st2.align(greedy(W, lib), pcm, ids)
            assert [a["id"] for a in al] == ids + [ctx.token_eot()] and al[-1]["t_dtw"] == -1
            out["%s_seed%d" % (tag, seed)] = (ids, t_full, [a["t_dtw"] for a in al[:-1]], n_seg)
            stats = [a + b for a, b in zip(stats, st.dtw_stats())]
            stats = [a + b for a, b in zip(stats, st2.dtw_stats())]
            st.free()
            st2.free()
        ctx.free()
    return out, stats


@pytest.fixture(scope="module")
def device_dtw(wrs, amd_lib):
    assert os.environ.get("WHISPER_AMD_DTW_HOST", "0") != "1", "the suite runs with the default DTW path"
    return dtw_runs(wrs, amd_lib)


def test_times_equal_full(device_dtw):
    runs, (n_dev, n_host, n_fall) = device_dtw
    assert len(runs) == len(cases.DTW_CASES) * len(SEEDS)
    for k, (ids, t_full, t_align, n_seg) in runs.items():
        assert len(ids) > 100 and len(t_full) == len(t_align) == len(ids), k
        assert any(t >= 0 for t in t_full), k                   # full() placed timestamps
        assert t_align == t_full, k
    assert n_dev == 2 * len(runs) and n_host == 0 and n_fall == 0, (n_dev, n_host, n_fall)


def test_times_equal_full_on_the_host_dtw_path(device_dtw):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, WHISPER_AMD_DTW_HOST="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert {k: tuple(v) for k, v in res["runs"].items()} == {k: tuple(v) for k, v in device_dtw[0].items()}
    assert res["stats"] == [0, device_dtw[1][0], 0], res["stats"]


# ---- 2. scores against the logits of whisper_amd_decode_batch --------------------------------------------------------------------------------
def logits_by_decode_batch(st, seq, sot_len):
    """rows sot_len .. len(seq) - 2 of the causal pass over seq, eight flagged rows a call (as many as a pass allows), every call the whole
    sequence on cleared cells.
    Extending a prefix call by call instead gives other bits, and has to: the reference's P V product (ggml_vec_dot_f16 over the cells
    in use) adds in 32 chains with a sequential tail, so a row's value depends on how many cells the PASS covers - 10 cells are all tail,
    64 cells are two full steps.  Measured on the MI355X with the prefix extended: rows 0..4 of the F16 s128 case within 1 ulp, row 5 228
    ulps off in plog.  align() is one pass over the whole sequence, as whisper_full's DTW pass is; so are these calls."""
    n, rows = len(seq), []
    for first in range(sot_len, n - 1, 8):
        st.kv_op(0)
        flags = [1 if first <= i < min(first + 8, n - 1) else 0 for i in range(n)]
        rows.append(st.decode_batch(seq, list(range(n)), [0] * n, flags))
    st.kv_op(0)
    return np.concatenate(rows)


def scored_against_logits(W, lib, name, n_take=60):
    """align() of full()'s own first n_take text ids on model `name`, and the float64 yardstick from decode_batch's logits"""
    ctx = W.WhisperContext.new_with_params(model_of(name), W.WhisperContextParameters(lib), lib=lib)
    pcm = wsynth.synth_audio(N_SAMPLES, 0)
    st = ctx.create_state()
    st.full(greedy(W, lib), pcm)
    ids = text_of(st, ctx.token_eot())[0][:n_take]
    assert len(ids) >= 20, (name, len(ids))
    before = st.align_stats()
    al = st.align(greedy(W, lib), pcm, ids)
    after = st.align_stats()
    lang = ctx.token_lang(lib.whisper_lang_id(b"en"))
    seq = [ctx.token_sot(), lang, ctx.token_not()] + ids + [ctx.token_eot()]
    st.pcm_to_mel(pcm)
    st.encode(0)
    logits = logits_by_decode_batch(st, seq, 2)
    want = align_cases.expected(logits, seq[3:])
    st.free()
    ctx.free()
    return ids, al, want, (before, after), logits.shape


def check_scores(name, ids, al, want, stats, shape):
    assert shape[0] == len(ids) + 1 == len(al) == len(want)
    worst = [0, 0, 0]
    for r, (a, w) in enumerate(zip(al, want)):
        plog, p, best, best_plog, _best_p, rank = w
        d = [align_cases.ulps32(a["plog"], plog), align_cases.ulps32(a["p"], p), align_cases.ulps32(a["best_plog"], best_plog)]
        worst = [max(x, y) for x, y in zip(worst, d)]
        assert a["best_id"] == best and a["rank"] == rank, (name, r, a, best, rank)
        assert max(d) <= 1, (name, r, d)
    print("%s: %d rows, worst ulps plog %d p %d best_plog %d" % (name, len(al), *worst))
    (c0, r0, b0), (c1, r1, b1) = stats
    assert (c1 - c0, r1 - r0, b1 - b0) == (1, len(al), len(al) * shape[1] * 4), stats


@pytest.fixture(scope="module")
def f16_scores(wrs, amd_lib):
    return scored_against_logits(wrs, amd_lib, "s128")


def test_scores_equal_the_models_logits_f16(f16_scores):
    check_scores("s128", *f16_scores)


@pytest.mark.parametrize("name", MODELS[1:])
def test_scores_equal_the_models_logits_quantised(wrs, amd_lib, name):
    check_scores(name, *scored_against_logits(wrs, amd_lib, name))


def test_scores_do_not_depend_on_timing(wrs, f16_scores):
    """the same on the build whose one-launch product waves stall at random (libwhisper_chaos.so): identical records"""
    path = os.path.join(ROOT, "whisper-rust_amd", "libwhisper_chaos.so")
    assert os.path.exists(path), "libwhisper_chaos.so missing: make -C whisper-rust_amd libwhisper_chaos.so (__graft_entry__.build() does)"
    lib = wrs.load_library(path)
    wrs.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    ids, al, want, stats, shape = scored_against_logits(wrs, lib, "s128")
    check_scores("s128 (stalled build)", ids, al, want, stats, shape)
    assert ids == f16_scores[0] and al == f16_scores[1]


# ---- 3. a better transcript scores better ----------------------------------------------------------------------------------------------------
def test_a_better_transcript_scores_better(wrs, amd_lib):
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcm = wsynth.synth_audio(N_SAMPLES, 0)
    st = ctx.create_state()
    st.full(greedy(wrs, amd_lib), pcm)
    ids = text_of(st, ctx.token_eot())[0]
    other = next(t for t in (1000, 1001, 1002) if t not in ids)
    worse = [other if i % 3 == 2 else t for i, t in enumerate(ids)]
    good, bad = st.align(greedy(wrs, amd_lib), pcm, ids), st.align(greedy(wrs, amd_lib), pcm, worse)
    s_good, s_bad = sum(a["plog"] for a in good[:-1]), sum(a["plog"] for a in bad[:-1])
    print("sum plog: greedy ids %.3f, every third replaced %.3f; greedy tokens of rank 0: %d of %d" % (s_good, s_bad, sum(a["rank"] == 0 for a in good[:-1]), len(ids)))
    assert s_good > s_bad
    assert any(a["rank"] == 0 and a["best_id"] == a["id"] for a in good[:-1])       # where no sampler rule decided, the greedy token is the model's own choice
    assert all((a["rank"] == 0) == (a["best_id"] == a["id"]) for a in good + bad)
    # the replaced tokens are not the model's choice, and the rows in front of them have not changed
    assert all(b["rank"] > 0 for i, b in enumerate(bad[:-1]) if i % 3 == 2)
    assert bad[0] == good[0] and bad[1] == good[1]
    st.free()
    ctx.free()


# ---- 4. refusals and hygiene -----------------------------------------------------------------------------------------------------------------
def test_refusals(wrs, amd_lib):
    mp = wsynth.model_path("s128")
    ctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcm = wsynth.synth_audio(N_SAMPLES, 0)
    st = ctx.create_state()
    fp = greedy(wrs, amd_lib)

    def code(pcm_, ids, st_=st, **kw):
        p = greedy(wrs, amd_lib)
        for k, v in kw.items():
            p.set(k, v)
        with pytest.raises(wrs.WhisperError) as e:
            st_.align(p, pcm_, ids)
        return e.value.code

    assert code(pcm, [100, ctx.token_eot(), 101]) == wrs.ALIGN_BAD_TOKEN
    assert code(pcm, [100, ctx.token_beg() + 5]) == wrs.ALIGN_BAD_TOKEN
    assert code(pcm, []) == wrs.ALIGN_NO_TOKENS
    assert code(pcm, [100] * ctx.n_text_ctx()) == wrs.ALIGN_TOO_LONG
    assert code(pcm, [100] * (ctx.n_text_ctx() - 3)) == wrs.ALIGN_TOO_LONG          # + sot, lang, not, eot: one row too many
    assert code(pcm[:1500], [100, 101]) == wrs.ALIGN_TOO_SHORT                         # 93 ms
    assert code(pcm, [100, 101], offset_ms=4950) == wrs.ALIGN_TOO_SHORT                # 50 ms after the offset
    fctx = wrs.WhisperContext.new_with_params(mp, wrs.WhisperContextParameters(amd_lib, flash_attn=True), lib=amd_lib)
    fst = fctx.create_state()
    assert code(pcm, [100, 101], st_=fst) == wrs.ALIGN_FLASH_ATTN
    fst.free()
    fctx.free()
    assert st.align_stats() == (0, 0, 0)
    # the longest sequence that fits is taken, and the state is as usable as before
    al = st.align(fp, pcm, [100] * (ctx.n_text_ctx() - 4))
    assert len(al) == ctx.n_text_ctx() - 3 and st.align_stats()[0] == 1
    st.free()
    ctx.free()


def test_state_hygiene(wrs, amd_lib):
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    pcm, pcm2 = wsynth.synth_audio(N_SAMPLES, 0), wsynth.synth_audio(N_SAMPLES, 2)
    fresh = ctx.create_state()
    fresh.full(greedy(wrs, amd_lib), pcm2)
    want2 = fresh.segments()
    fresh.free()

    st = ctx.create_state()
    st.full(greedy(wrs, amd_lib), pcm)
    segs = st.segments()
    ids = text_of(st, ctx.token_eot())[0][:40]
    al = st.align(greedy(wrs, amd_lib), pcm, ids)
    assert st.segments() == segs                                    # result_all untouched
    assert all(a["t_dtw"] == -1 for a in al)                        # a context without alignment heads: scores only
    assert st.dtw_stats() == (0, 0, 0)
    # device-pointer samples: the audio front end leaves them in a buffer of the state
    dptr, n = st.audio_to_pcm(pcm, 1, 16000)
    assert n == len(pcm) and st.align(greedy(wrs, amd_lib), (dptr, n), ids) == al
    # align_text: the tokenizer's ids
    text = b"".join(ctx.token_to_bytes(t) for t in ids).decode(errors="replace")
    toks = ctx.tokenize(text)
    if toks and all(0 <= t < ctx.token_eot() for t in toks) and len(toks) + 4 <= ctx.n_text_ctx():
        assert [a["id"] for a in st.align_text(greedy(wrs, amd_lib), pcm, text)] == toks + [ctx.token_eot()]
    # a window further in: offset_ms moves the encoder, and the scores differ
    off = st.align(wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0, offset_ms=2000), pcm, ids)
    assert [a["id"] for a in off] == [a["id"] for a in al] and off != al
    assert st.segments() == segs
    st.free()
    # align() on a state that has done nothing else gives the same records, and full() after it the segments of a fresh state.  (Not on `st`
    # above: whisper_full's no_speech_prob reads row 0 of the state's host logits as the LAST call left it - the reference's own quirk,
    # wa_full.cpp - so a second full() on any state differs there from a fresh state's, with or without an align() between them.  align()
    # does not write those logits, which this comparison shows.)
    st = ctx.create_state()
    assert st.align(greedy(wrs, amd_lib), pcm, ids) == al
    assert st.full_n_segments() == 0
    st.full(greedy(wrs, amd_lib), pcm2)
    got2 = st.segments()
    for a, b in zip(got2, want2):
        print("keys that differ from the fresh state's segment:", [k for k in a if a[k] != b[k]])
    assert got2 == want2
    st.free()
    ctx.free()


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "child":
    import whisper_rs as W_
    lib_ = W_.load_library()
    W_.set_log_callback(lib_, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    runs_, stats_ = dtw_runs(W_, lib_)
    print(json.dumps(dict(runs=runs_, stats=stats_)))

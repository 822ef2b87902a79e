"""The int8 matrix-core kernel of the K formats (wa_quantk_mfma.hip: k_kgemm_mfma) through the C ABI: Q2_K / Q3_K / Q5_K / Q6_K models whose products of
more than 8 rows - the encoder, the cross K/V product, prompt passes, DTW's extra decoder pass - it now serves, counted by whisper_amd_qgemm_stats.

  * s256:q5_k / q6_k / q2_k / q3_k (1 and 4 blocks per row; the encoder's products take the kernel's four-rows-per-lane form, prompt passes the
    one-row form): after pcm_to_mel + encode(0) the counter shows products served by the matrix-core kernel and none by k_kgemm_exact,
    and the encoder output's digest is the reference engine's (tests/golden/s256_kquant.json / s256_kquant23.json, the model file's hash
    checked against the golden's);
  * m1024:q6_k (4 and 16 blocks per row) beside oracle/_ref/libwhisper_ref.so live on the same file;
  * s256:q5_k and s256:q2_k: teacher-forced prompt passes of 12 and of 40 tokens at n_past 0 and a single token behind each: the logits digests
    equal the reference engine's live, and the counter grows by the products of a pass (six per decoder layer) - by nothing for the single token;
  * WHISPER_AMD_NO_QMFMA=1 (read once per process: a fresh child process runs the same script) sends every such product to k_kgemm_exact and
    changes no digest;
  * a greedy full() with DTW token timestamps (N_TOP_MOST) on s256:q6_k: segments and t_dtw equal the run under the switch.
Everything is equality of digests, token lists or counters."""
import ctypes as C
import hashlib
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

import wsynth  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLDEN_FILE = {"q5_k": "s256_kquant.json", "q6_k": "s256_kquant.json", "q2_k": "s256_kquant23.json", "q3_k": "s256_kquant23.json"}
MODEL_CASES = ("s256:q5_k", "s256:q6_k", "s256:q2_k", "s256:q3_k", "m1024:q6_k")
LIVE_MODEL = "m1024:q6_k"
PROMPT_MODELS = ("s256:q5_k", "s256:q2_k")
PROMPT_LENGTHS = (12, 40)
DTW_MODEL = ("s256", "q6_k")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def prompt(ctx, n):
    return [ctx.token_sot()] + [(1000 + 977 * i) % 50000 for i in range(n - 1)]


def embd_enc(lib, st, n, fn="whisper_amd_get_embd_enc"):
    f = getattr(lib, fn)
    out = np.empty(n, np.float32)
    if fn == "whisper_amd_get_embd_enc":
        f.restype = C.c_int64
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int64]
        assert f(st.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n) == n
    else:
        f.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
        f(st.ptr, out.ctypes.data_as(C.POINTER(C.c_float)), n)
    return out


def segs(st):
    return [dict(t0=s["t0"], t1=s["t1"], ids=s["ids"], t_dtw=s["t_dtw"]) for s in st.segments()]


def run_script(W, lib, product=True):
    """The script of this file on one library: per model the encoder output's digest (and, on the product, the counter after encode); for the prompt
    models the logits digests of the prompt passes and of the single token behind each (and how the counter grew); on the product the DTW run."""
    th = {} if product else {"n_threads": 16}
    out = {}
    pcm = wsynth.synth_audio(480000, 0)
    for name in MODEL_CASES:
        if not product and name not in PROMPT_MODELS and name != LIVE_MODEL:
            continue
        mp = wsynth.quant_model_path(*name.split(":"))
        ctx = W.WhisperContext.new_with_params(mp, W.WhisperContextParameters(lib) if product else W.WhisperContextParameters(lib, use_gpu=False), lib=lib)
        st = ctx.create_state()
        if product:
            st.pcm_to_mel(pcm); st.encode(0)
        else:
            st.pcm_to_mel(pcm, 8); st.encode(0, 16)
        d = ctx.model_n_audio_state()
        rec = dict(embd=digest(embd_enc(lib, st, 1500 * d, "whisper_amd_get_embd_enc" if product else "ref_shim_get_embd_enc")),
                   n_text_layer=ctx.model_n_text_layer())
        if product:
            rec["after_encode"] = list(st.qgemm_stats())
        if name in PROMPT_MODELS:
            rec["passes"] = []
            for n in PROMPT_LENGTHS:
                s0 = st.qgemm_stats() if product else (0, 0)
                st.decode(prompt(ctx, n), 0, **th)
                lg = digest(st.get_logits_last(n))
                s1 = st.qgemm_stats() if product else (0, 0)
                st.decode([ctx.token_beg() + 7], n, **th)
                lg1 = digest(st.get_logits_last(1))
                s2 = st.qgemm_stats() if product else (0, 0)
                rec["passes"].append(dict(n=n, prompt=lg, single=lg1, grew=[s1[0] - s0[0], s1[1] - s0[1]], grew_single=[s2[0] - s1[0], s2[1] - s1[1]]))
        st.free(); ctx.free()
        out[name] = rec
    if product:
        ctx = W.WhisperContext.new_with_params(wsynth.quant_model_path(*DTW_MODEL), W.WhisperContextParameters(lib, dtw_preset=W.AHEADS_N_TOP_MOST, dtw_n_top=2),
                                               lib=lib)
        st = ctx.create_state()
        st.full(W.FullParams(lib, 0, best_of=1, temperature_inc=0.0), pcm)
        out["dtw"] = dict(segments=segs(st), stats=list(st.qgemm_stats()), dtw_stats=list(st.dtw_stats()))
        st.free(); ctx.free()
    return out


@pytest.fixture(scope="module")
def product_run(wrs, amd_lib):
    assert os.environ.get("WHISPER_AMD_NO_QMFMA") is None, "the suite runs with the default routing"
    assert hasattr(amd_lib, "whisper_amd_qgemm_stats"), "whisper_amd_qgemm_stats is not exported"
    return run_script(wrs, amd_lib)


@pytest.fixture(scope="module")
def reference_run(wrs, ref_lib):
    return run_script(wrs, ref_lib, product=False)


@pytest.mark.parametrize("name", MODEL_CASES)
def test_encoder_runs_on_the_matrix_cores_and_equals_the_reference(request, product_run, name):
    rec = product_run[name]
    assert rec["after_encode"][0] > 0 and rec["after_encode"][1] == 0, rec["after_encode"]
    shape, qt = name.split(":")
    if name != LIVE_MODEL:
        gold = json.load(open(os.path.join(GOLDEN, GOLDEN_FILE[qt])))[qt]
        assert hashlib.sha256(open(wsynth.quant_model_path(shape, qt), "rb").read()).hexdigest() == gold["model_sha256"], "the quantised model file differs from the goldens'"
        assert rec["embd"] == gold["embd_enc"]["sha256"], name
    else:
        assert rec["embd"] == request.getfixturevalue("reference_run")[name]["embd"], name


@pytest.mark.parametrize("name", PROMPT_MODELS)
def test_prompt_passes_equal_the_reference_and_are_counted(product_run, reference_run, name):
    rec, ref = product_run[name], reference_run[name]
    assert rec["embd"] == ref["embd"], name
    for got, want in zip(rec["passes"], ref["passes"]):
        assert got["prompt"] == want["prompt"], (name, got["n"])
        assert got["single"] == want["single"], (name, got["n"])
        assert got["grew"] == [6 * rec["n_text_layer"], 0], (name, got)          # q|k|v, out, cross q, cross out, fc1, fc2 of every layer
        assert got["grew_single"] == [0, 0], (name, got)                         # products of one row are not counted
    assert len(rec["passes"]) == len(PROMPT_LENGTHS) == len(ref["passes"])


@pytest.fixture(scope="module")
def switched_run():
    """the switch is read once per process: a child process starts with it set"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, WHISPER_AMD_NO_QMFMA="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_switch_goes_back_to_the_general_kernel(product_run, switched_run):
    for name in MODEL_CASES:
        a, b = product_run[name], switched_run[name]
        assert b["after_encode"][0] == 0 and b["after_encode"][1] == a["after_encode"][0] > 0, (name, a["after_encode"], b["after_encode"])
        assert a["embd"] == b["embd"], name
        for pa, pb in zip(a.get("passes", []), b.get("passes", [])):
            assert (pa["prompt"], pa["single"]) == (pb["prompt"], pb["single"]), (name, pa["n"])
            assert pb["grew"] == [0, pa["grew"][0]] and pb["grew_single"] == [0, 0], (name, pb)


def test_dtw_token_timestamps_do_not_change(product_run, switched_run):
    a, b = product_run["dtw"], switched_run["dtw"]
    assert a["segments"] == b["segments"] and a["segments"]
    assert any(t != -1 for s in a["segments"] for t in s["t_dtw"])          # timestamps were placed
    assert a["dtw_stats"][0] + a["dtw_stats"][1] > 0                          # the extra decoder pass ran
    assert a["stats"][0] > 0 and a["stats"][1] == 0 and b["stats"] == [0, a["stats"][0]], (a["stats"], b["stats"])


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "child":
    import whisper_rs as W_
    lib_ = W_.load_library()
    W_.set_log_callback(lib_, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    print(json.dumps(run_script(W_, lib_)))

"""The few-rows kernel of the K formats (wa_quantk_rows.hip: k_kgemv_rows) through the C ABI: Q2_K / Q3_K / Q5_K / Q6_K models whose products of 2..8
rows - beam-search and best_of steps, small whisper_decode batches - it now takes, counted by whisper_amd_few_rows_stats (which counts the 32-value
formats' k_qgemv_rows too).

  * s256:q5_k / q6_k (tests/golden/s256_kquant.json) and s256:q2_k / q3_k (s256_kquant23.json), read only: the `ladder` and `beam3` runs and the logits
    digest of the 5-token batch equal the reference engine's goldens; afterwards the counter shows products taken by the few-rows kernel and none
    of 2..8 rows by the general kernel, and both one-launch forms are still off;
  * live beside the reference engine (oracle/_ref/libwhisper_ref.so) on s256:q5_k and s256:q2_k: beam 5 and beam 8 full() with max_tokens = 32 and
    temperature_inc = 0 give identical segments / ids / p / plog, whisper_decode batches of 2, 5 and 8 tokens equal logits digests;
  * WHISPER_AMD_NO_FEW_ROWS=1 is read once per process: a fresh child process with it runs the same beam-3 runs - same segments, no product taken by
    the few-rows kernel, all of them by the general one;
  * s128:q5_1, a 32-value model: beam 3 is counted too.
Everything is equality of bytes or of token lists; the counts are per graph capture, so they are compared with zero only."""
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
LIVE = ("q5_k", "q2_k")
FULL = {"ladder": dict(strategy=0, best_of=2, temperature_inc=0.2), "beam3": dict(strategy=1, beam_size=3, best_of=2, temperature_inc=0.0)}      # tools/gen_golden_quant.py: FULL
BATCH = (5, 5)          # the goldens' 5-token batch: (tokens, n_past)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def segs(st):
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"], tids=s["tids"],
                 p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]]) for s in st.segments()]


def params(W, lib, kw, **extra):
    kk = {k: v for k, v in kw.items() if k != "strategy"}
    kk.update(extra)
    return W.FullParams(lib, kw.get("strategy", 0), **kk)


def gold_of(qt):
    return json.load(open(os.path.join(GOLDEN, GOLDEN_FILE[qt])))[qt]


def golden_script(W, lib, only=None):
    """Per K format on the product: the segments of the golden runs in `only` (default: all of FULL), the counter after each, the logits digest of
    the goldens' teacher-forced sequence up to its 5-token batch, and the one-launch switches of the beam state."""
    lib.whisper_amd_mega_enabled.argtypes = [C.c_void_p]
    lib.whisper_amd_rows_enabled.argtypes = [C.c_void_p]
    out = {}
    pcm = wsynth.synth_audio(480000, 0)
    for qt in GOLDEN_FILE:
        ctx = W.WhisperContext.new_with_params(wsynth.quant_model_path("s256", qt), W.WhisperContextParameters(lib), lib=lib)
        rec = {}
        for tag in (only or FULL):
            st = ctx.create_state()
            st.full(params(W, lib, FULL[tag]), pcm)
            rec[tag] = dict(segments=segs(st), stats=list(st.few_rows_stats()), forms=[lib.whisper_amd_mega_enabled(st.ptr), lib.whisper_amd_rows_enabled(st.ptr)],
                            rows_stats=list(st.rows_stats()))
            st.free()
        if only is None:
            st = ctx.create_state()
            st.pcm_to_mel(pcm); st.encode(0)
            for e in gold_of(qt)["logits"]:
                st.decode(e["tokens"], e["n_past"])
                if (len(e["tokens"]), e["n_past"]) == BATCH:
                    rec["batch"] = dict(sha256=digest(st.get_logits_last(len(e["tokens"]))), stats=list(st.few_rows_stats()))
                    break
            st.free()
        ctx.free()
        out[qt] = rec
    return out


@pytest.fixture(scope="module")
def product_run(wrs, amd_lib):
    assert os.environ.get("WHISPER_AMD_NO_FEW_ROWS") is None, "the suite runs with the default routing"
    assert hasattr(amd_lib, "whisper_amd_few_rows_stats"), "whisper_amd_few_rows_stats is not exported"
    return golden_script(wrs, amd_lib)


@pytest.mark.parametrize("qt", list(GOLDEN_FILE))
def test_goldens_through_the_few_rows_kernel(product_run, qt):
    gold, rec = gold_of(qt), product_run[qt]
    assert hashlib.sha256(open(wsynth.quant_model_path("s256", qt), "rb").read()).hexdigest() == gold["model_sha256"], "the quantised model file differs from the goldens'"
    for tag in FULL:
        assert rec[tag]["segments"] == gold["full"]["%s_seed0" % tag], (qt, tag)
        assert rec[tag]["stats"][1] == 0, (qt, tag, rec[tag]["stats"])               # no product of 2..8 rows went to the general kernel
        assert rec[tag]["forms"] == [0, 0] and rec[tag]["rows_stats"] == [0, 0], (qt, tag, rec[tag])      # not a one-launch form
    want = [e for e in gold["logits"] if (len(e["tokens"]), e["n_past"]) == BATCH]
    assert len(want) == 1 and rec["batch"]["sha256"] == want[0]["sha256"], qt
    assert rec["beam3"]["stats"][0] > 0, (qt, rec["beam3"]["stats"])                   # a beam step is three rows
    assert rec["batch"]["stats"][0] > 0 and rec["batch"]["stats"][1] == 0, (qt, rec["batch"]["stats"])


LIVE_BATCHES = (([50258, 50259, 50359], 0), ([4321, 777], 3), ([31000, 15, 50, 1200, 77], 5), ([9, 4000, 25000, 333, 50100, 7, 1234, 42], 10))      # 3 to fill, then 2, 5, 8


def live_script(W, lib, product):
    th = {} if product else {"n_threads": 16}
    out = {}
    pcm = wsynth.synth_audio(480000, 0)
    for qt in LIVE:
        mp = wsynth.quant_model_path("s256", qt)
        ctx = W.WhisperContext.new_with_params(mp, W.WhisperContextParameters(lib) if product else W.WhisperContextParameters(lib, use_gpu=False), lib=lib)
        rec = {}
        for beam in (5, 8):
            st = ctx.create_state()
            st.full(W.FullParams(lib, 1, beam_size=beam, temperature_inc=0.0, max_tokens=32, **th), pcm)
            rec["beam%d" % beam] = segs(st)
            if product:
                rec["beam%d_stats" % beam] = list(st.few_rows_stats())
            st.free()
        st = ctx.create_state()
        if product:
            st.pcm_to_mel(pcm); st.encode(0)
        else:
            st.pcm_to_mel(pcm, 8); st.encode(0, 16)
        rec["batches"] = []
        for toks, n_past in LIVE_BATCHES:
            if product:
                st.decode(toks, n_past)
            else:
                st.decode(toks, n_past, 16)
            rec["batches"].append(digest(st.get_logits_last(len(toks))))
        st.free(); ctx.free()
        out[qt] = rec
    return out


@pytest.fixture(scope="module")
def product_live(wrs, amd_lib):
    return live_script(wrs, amd_lib, True)


@pytest.fixture(scope="module")
def reference_live(wrs, ref_lib):
    return live_script(wrs, ref_lib, False)


@pytest.mark.parametrize("qt", LIVE)
def test_beams_and_batches_live_beside_the_reference(product_live, reference_live, qt):
    got, want = product_live[qt], reference_live[qt]
    for beam in (5, 8):
        assert got["beam%d" % beam] and got["beam%d" % beam] == want["beam%d" % beam], (qt, beam)
    st = got["beam5_stats"]
    assert st[0] > 0 and st[1] == 0, (qt, st)          # (steps of 8 rows at this width are the general kernel's by the default rule)
    assert [len(t) for t, _ in LIVE_BATCHES] == [3, 2, 5, 8]
    assert got["batches"] == want["batches"], qt


@pytest.fixture(scope="module")
def switched_run():
    """the switch is read once per process: a child process starts with it set"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child"], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, WHISPER_AMD_NO_FEW_ROWS="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_the_switch_goes_back_to_the_general_kernel(product_run, switched_run):
    for qt in GOLDEN_FILE:
        a, b = product_run[qt]["beam3"], switched_run[qt]["beam3"]
        assert a["segments"] == b["segments"] and a["segments"], qt
        assert b["stats"][0] == 0 and b["stats"][1] > 0, (qt, b["stats"])


def test_a_32_value_model_is_counted_too(wrs, amd_lib):
    """s128:q5_1, beam 3: k_qgemv_rows takes its beam steps and the same counter shows it."""
    ctx = wrs.WhisperContext.new_with_params(wsynth.quant_model_path("s128", "q5_1"), wrs.WhisperContextParameters(amd_lib), lib=amd_lib)
    st = ctx.create_state()
    st.full(wrs.FullParams(amd_lib, 1, beam_size=3, temperature_inc=0.0), wsynth.synth_audio(480000, 0))
    stats = st.few_rows_stats()
    assert st.segments() and stats[0] > 0, stats
    st.free(); ctx.free()


if __name__ == "__main__" and len(sys.argv) > 1 and sys.argv[1] == "child":
    import whisper_rs as W_
    lib_ = W_.load_library()
    W_.set_log_callback(lib_, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    print(json.dumps(golden_script(W_, lib_, only=("beam3",))))

"""DTW token timestamps through full(): the device path (wa_dtw.hip on the state's stream) is what a state takes by default, the host path
(WHISPER_AMD_DTW_HOST=1, read when a state is created) gives the same segments and t_dtw, both equal the reference engine's goldens
(tests/golden/s128.json "dtw"), and two states of one context running their DTW passes at the same time do not disturb each other."""
import json
import os
import subprocess
import sys
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"), os.path.join(ROOT, "whisper-rust_amd")):      # (the child process below runs this file as a script)
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gen_golden_cases as cases  # noqa: E402
import wsynth  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
SEEDS = (0, 1)


def segs(st):
    return [dict(t0=s["t0"], t1=s["t1"], ids=s["ids"], t_dtw=s["t_dtw"]) for s in st.segments()]


def run_cases(W, lib, mp):
    """every s128 DTW golden case on a fresh state: {tag_seed: segments}, and the states' DTW counters summed"""
    out, stats = {}, [0, 0, 0]
    for tag, preset, kw in cases.DTW_CASES:
        ctx = W.WhisperContext.new_with_params(mp, W.WhisperContextParameters(lib, dtw_preset=preset, **kw), lib=lib)
        for aseed in SEEDS:
            st = ctx.create_state()
            st.full(W.FullParams(lib, 0, best_of=1, temperature_inc=0.0), wsynth.synth_audio(480000, aseed))
            out["%s_seed%d" % (tag, aseed)] = segs(st)
            stats = [a + b for a, b in zip(stats, st.dtw_stats())]
            st.free()
        ctx.free()
    return out, stats


@pytest.fixture(scope="module")
def gold():
    g = json.load(open(os.path.join(GOLDEN, "s128.json")))
    return g, wsynth.model_path("s128", g["model_seed"])


@pytest.fixture(scope="module")
def device_run(wrs, amd_lib, gold):
    assert os.environ.get("WHISPER_AMD_DTW_HOST", "0") != "1", "the suite runs with the default DTW path"
    return run_cases(wrs, amd_lib, gold[1])


def test_device_path_is_the_default_and_matches_the_goldens(device_run, gold):
    got, (n_dev, n_host, n_fall) = device_run
    assert got == {k: gold[0]["dtw"][k] for k in got} and len(got) == len(cases.DTW_CASES) * len(SEEDS)
    assert any(t != -1 for ss in got.values() for s in ss for t in s["t_dtw"])          # timestamps were placed
    assert n_dev > 0 and n_host == 0 and n_fall == 0, (n_dev, n_host, n_fall)


def test_host_path_switch_gives_the_same(device_run, gold):
    """the switch is read when a state is created; a child process starts with it set"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", gold[1]], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, WHISPER_AMD_DTW_HOST="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["segments"] == device_run[0]
    assert res["segments"] == {k: gold[0]["dtw"][k] for k in res["segments"]}
    n_dev, n_host, n_fall = res["stats"]
    assert n_dev == 0 and n_host == device_run[1][0] and n_fall == 0, res["stats"]


def test_two_states_at_the_same_time(wrs, amd_lib, gold, device_run):
    tag, preset, kw = cases.DTW_CASES[0]
    ctx = wrs.WhisperContext.new_with_params(gold[1], wrs.WhisperContextParameters(amd_lib, dtw_preset=preset, **kw), lib=amd_lib)
    sts = [ctx.create_state() for _ in SEEDS]
    pcm = [wsynth.synth_audio(480000, s) for s in SEEDS]
    fps = [wrs.FullParams(amd_lib, 0, best_of=1, temperature_inc=0.0) for _ in SEEDS]
    err = []

    def work(i):
        try:
            sts[i].full(fps[i], pcm[i])
        except Exception as e:      # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(i,)) for i in range(len(SEEDS))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not err, err
    for i, s in enumerate(SEEDS):
        assert segs(sts[i]) == device_run[0]["%s_seed%d" % (tag, s)], s           # = the solo run
        n_dev, n_host, n_fall = sts[i].dtw_stats()
        assert n_dev > 0 and n_host == 0 and n_fall == 0
        sts[i].free()
    ctx.free()


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "child":
    import whisper_rs as W
    lib_ = W.load_library()
    W.set_log_callback(lib_, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    got_, stats_ = run_cases(W, lib_, sys.argv[2])
    print(json.dumps(dict(segments=got_, stats=stats_)))

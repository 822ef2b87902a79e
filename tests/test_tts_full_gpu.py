"""full() with token_timestamps on the device path (whisper-rust_amd/csrc/wa_tts.cpp), s128 model, the audio seeds of tests/golden/s128_token_ts.json:
token t0 / t1 / vlen and the segments, with and without max_len and split_on_word (the goldens' three cases, and max_len = 1 with split_on_word),
must equal the goldens where there are some and the host path's (WHISPER_AMD_TTS_HOST=1 is read once per process: a child runs this file as a
script); PCM that lies in HBM is not copied back; the members of a lock-step wave get their solo times."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "whisper-rust_amd")]      # (the child process has no conftest)
import gen_golden_tts as G  # noqa: E402
import whisper_rs as W  # noqa: E402
import wsynth  # noqa: E402

CASES = dict(G.TTS_CASES, token_ts_one_word=dict(best_of=1, temperature_inc=0.0, token_timestamps=True, max_len=1, split_on_word=True))
SEEDS = (0, 1)


def run_cases(lib):
    """{case_seed: segments}, and the token-timestamp counters summed over the states"""
    ctx = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(lib), lib=lib)
    out, stats = {}, {}
    for tag, kw in CASES.items():
        for seed in SEEDS:
            st = ctx.create_state()
            st.full(W.FullParams(lib, 0, **kw), wsynth.synth_audio(480000, seed))
            out["%s_seed%d" % (tag, seed)] = G.segs(st)
            for k, v in st.tts_stats().items():
                stats[k] = stats.get(k, 0) + v
            st.free()
    ctx.free()
    return out, stats


if __name__ == "__main__":
    json.dump(run_cases(W.load_library(os.path.join(ROOT, "whisper-rust_amd", "libwhisper.so"))), sys.stdout)
    sys.exit(0)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device_run(amd_lib):
    assert os.environ.get("WHISPER_AMD_TTS_HOST") != "1"
    return run_cases(amd_lib)


@pytest.fixture(scope="module")
def host_run():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, WHISPER_AMD_TTS_HOST="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("tag", list(CASES))
def test_device_path_equals_host_path_and_goldens(device_run, host_run, tag, seed):
    n, key = len(CASES) * len(SEEDS), "%s_seed%d" % (tag, seed)
    assert device_run[1] == dict(device_run[1], energy_launches=n, fallbacks=0, bytes_d2h=0) and device_run[1]["snap_launches"] >= n
    assert host_run[1] == dict(energy_launches=0, snap_launches=0, fallbacks=0, bytes_d2h=0)            # each process took its path
    got = device_run[0][key]
    assert sum(len(s["ids"]) for s in got) > 10 and any(a != b for s in got for a, b in zip(s["tok_t0"], s["tok_t1"]))
    assert got == host_run[0][key]
    assert tag not in G.TTS_CASES or got == json.load(open(os.path.join(ROOT, "tests", "golden", "s128_token_ts.json")))[key]
    assert tag != "token_ts_one_word" or len(got) > len(device_run[0]["token_ts_seed%d" % seed])


def test_device_resident_pcm_is_not_copied_back(amd_lib, device_run):
    """whisper_amd_full_audio leaves the 16 kHz PCM in HBM and hands it to full() there"""
    ctx = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(amd_lib), lib=amd_lib)
    st = ctx.create_state()
    st.full_audio(W.FullParams(amd_lib, 0, **CASES["token_ts"]), wsynth.synth_audio(480000, 0), 1, 16000)
    stats = st.tts_stats()
    assert stats["bytes_d2h"] == 0 and stats["energy_launches"] >= 1 and stats["snap_launches"] >= 1 and stats["fallbacks"] == 0, stats
    assert G.segs(st) == device_run[0]["token_ts_seed0"]
    st.free(); ctx.free()


def test_lock_step_members_get_their_solo_times(amd_lib):
    ctx = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(amd_lib), lib=amd_lib)
    fp = W.FullParams(amd_lib, 0, **CASES["token_ts"])
    pcms = [wsynth.synth_audio(480000, seed) for seed in (0, 1, 2, 3)]
    solo, states = [ctx.create_state() for _ in pcms], [ctx.create_state() for _ in pcms]
    for st, pcm in zip(solo, pcms):
        st.full(fp, pcm)
    W.full_batch(ctx, states, fp, pcms)
    for k, (st, alone) in enumerate(zip(states, solo)):
        assert G.segs(st) == G.segs(alone) and len(G.segs(alone)) > 0, k
        assert st.tts_stats() == dict(st.tts_stats(), energy_launches=1, fallbacks=0, bytes_d2h=0)
        st.free(); alone.free()
    ctx.free()

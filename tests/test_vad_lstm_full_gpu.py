"""The device recurrence (k_vad_lstm) behind the public calls: whisper_vad_detect_speech over slabs, and a poll tick of two live
sessions.  Either path of a context - device, or host with WHISPER_AMD_VAD_LSTM_HOST=1 - gives the recorded probabilities of the reference
engine (tests/golden/vad.json); the contexts are made in fresh child processes, which read both variables when they create them."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
from conftest import GOLDEN
import wsynth
import wsynth_vad as V
import gen_golden_stream_vad as GG
import stream_vad_ref as R

pytestmark = pytest.mark.gpu

SLAB = 64


def bits(x):
    return [int(b) for b in np.ascontiguousarray(x, np.float32).view(np.uint32)]


def session_audios():
    x = GG.recording()
    return [x, np.concatenate([np.zeros(1700, np.float32), x])[:len(x)]]


def child_main():
    import whisper_rs as W
    v = W.WhisperVadContext.new(V.model_path(), lib=W.load_library())
    print("RESULT " + json.dumps(dict(path=v.lstm_path(), probs=bits(v.detect_speech(V.synth_audio())), stats=v.lstm_stats(),
                                      sessions=[bits(v.detect_speech(a)) for a in session_audios()])))
    v.free()


@pytest.fixture(scope="module")
def runs():
    def child(host):
        env = dict(os.environ, WHISPER_AMD_VAD_SLAB=str(SLAB), WHISPER_AMD_VAD_LSTM_HOST="1" if host else "0")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    return dict(device=child(False), host=child(True))


@pytest.mark.parametrize("path", ["device", "host"])
def test_detect_speech_on_either_path(runs, path):
    golden, got = json.load(open(os.path.join(GOLDEN, "vad.json")))["probs"]["full"], runs[path]
    n = len(golden["bits"])
    assert n == 438 and got["probs"] == golden["bits"], "the reference engine's probabilities"
    want = [1, -(-n // SLAB), n] if path == "device" else [0, 0, 0]           # the path, one launch per slab, every window
    assert [got["path"]] + got["stats"][:2] == want and (got["stats"][2] > 0) == (path == "device")


def test_two_sessions_share_a_recurrence_launch(wrs, amd_lib, runs):
    """a poll tick of two sessions: one launch; the probabilities of the host-path child, as many utterances as the offline restatement cuts"""
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, flash_attn=False), lib=amd_lib)
    vctx = wrs.WhisperVadContext.new(V.model_path(), lib=amd_lib)
    try:
        audios = session_audios()
        ss = [wrs.WhisperVadStream(ctx, vctx, vad_on_feed=0) for _ in audios]
        for s, a in zip(ss, audios):
            assert s.feed(a) == 0
        before = vctx.lstm_stats()
        wrs.stream_vad_poll_many(ss)
        after = vctx.lstm_stats()
        assert after[0] - before[0] == 1 and after[1] - before[1] == 2 * (len(audios[0]) // 512), "one launch, both sessions' whole windows"
        [s.flush() for s in ss]
        due = wrs.stream_vad_poll_many(ss)
        want = [R.segments(np.array(p, np.uint32).view(np.float32), GG.VAD) for p in runs["host"]["sessions"]]
        assert [bits(s.probs()) for s in ss] == runs["host"]["sessions"] and due == sum(len(w) for w in want) and all(len(w) >= 4 for w in want)
        assert [s.pending() for s in ss] == [len(w) for w in want]
        [s.close() for s in ss]
    finally:
        vctx.free()
        ctx.free()


if __name__ == "__main__" and "--child" in sys.argv:
    child_main()

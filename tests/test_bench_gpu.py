"""bench.py on the GPU (MI355X): a plain run times only the headline, and --dump-outputs writes exactly what full() returned to its
caller in the last timed step (segments and token data of the chunk, float64)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wsynth
from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_dump_outputs_are_what_full_returns(wrs, amd_lib, tmp_path):
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "s128", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], capture_output=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-1500:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    j = json.loads(lines[0])
    assert j["steps"] == 2 and j["warmup"] == 1 and j["ms_per_step"] > 0 and j["value"] > 0
    assert "roofline" not in j and "cpu_baseline" not in j and "flash_attn_path" not in j      # those need --full
    assert sorted(os.listdir(out_dir)) == ["chunk0_segments.npy", "chunk0_text.npy", "chunk0_tokens.npy"]
    segs, toks, text = (np.load(out_dir / ("chunk0_%s.npy" % n)) for n in ("segments", "tokens", "text"))
    assert segs.dtype == toks.dtype == text.dtype == np.float64 and segs.shape[1] == 5 and toks.shape[1] == 11

    # the same calls in this process: the bench's FullParams, the chunk's audio (seed = chunk id 0), PCM from the host, and one state for the
    # warm-up step and both timed steps (the no-speech probe of a call reads the logits the previous call left behind, as in the reference)
    ctx = wrs.WhisperContext.new_with_params(wsynth.model_path("s128"), wrs.WhisperContextParameters(amd_lib, gpu_device=0), lib=amd_lib)
    st = ctx.create_state()
    fp, pcm = wrs.FullParams(amd_lib, best_of=1, temperature_inc=0.0, language="en", no_context=True), wsynth.synth_audio(480000, 0)
    for _ in range(1 + 2):
        st.full(fp, pcm)
    want = st.segments()
    assert len(want) > 0
    want_segs = [[s["t0"], s["t1"], len(s["ids"]), s["no_speech_prob"], len(s["text"])] for s in want]
    want_toks = [[i, s["ids"][n], s["tids"][n], s["p"][n], s["plog"][n], s["pt"][n], s["ptsum"][n], s["tok_t0"][n], s["tok_t1"][n], s["t_dtw"][n], s["vlen"][n]]
                 for i, s in enumerate(want) for n in range(len(s["ids"]))]
    assert np.array_equal(segs, np.asarray(want_segs, dtype=np.float64), equal_nan=True)
    assert np.array_equal(toks, np.asarray(want_toks, dtype=np.float64), equal_nan=True)
    assert bytes(text.astype(np.uint8)) == b"".join(s["text"] for s in want)
    st.free()
    ctx.free()

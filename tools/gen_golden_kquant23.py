#!/usr/bin/env python3
"""Golden vectors for Q2_K and Q3_K: the REFERENCE ENGINE itself on the s256 synthetic model (d = 256, the smallest width whose rows hold
256-value blocks) quantised to Q2_K and Q3_K by the reference's own quantizer.  Same content as tests/golden/s256_kquant.json
(tools/gen_golden_kquant.py): digests of the encoder output and of teacher-forced logits, full transcriptions (greedy, temperature
ladder, beam) and the streaming pattern.  Every full() run recorded must hold at least 10 distinct token ids: a run that has collapsed
onto a few tokens shows little.  Needs the reference engine built (oracle/_ref); writes tests/golden/s256_kquant23.json."""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import wsynth  # noqa: E402
import whisper_rs as W  # noqa: E402
from gen_golden_quant import FULL, SEQS, digest, segs, stream_run  # noqa: E402

QTYPES = ("q2_k", "q3_k")
MIN_DISTINCT = 10

if __name__ == "__main__":
    ref = W.load_library(os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so"))
    W.set_log_callback(ref, None)
    ref.ref_shim_get_embd_enc.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.c_int]
    gold = {}
    for qt in QTYPES:
        mp = wsynth.quant_model_path("s256", qt)
        ctx = W.WhisperContext.new_with_params(mp, W.WhisperContextParameters(ref, use_gpu=False), lib=ref)
        d = ctx.model_n_audio_state()
        g = dict(model_bytes=os.path.getsize(mp), model_sha256=hashlib.sha256(open(mp, "rb").read()).hexdigest())
        st = ctx.create_state()
        st.pcm_to_mel(wsynth.synth_audio(480000, 0), 4); st.encode(0, 8)
        x = np.empty(1500 * d, np.float32)
        ref.ref_shim_get_embd_enc(st.ptr, x.ctypes.data_as(C.POINTER(C.c_float)), x.size)
        g["embd_enc"] = dict(sha256=digest(x), absmax=float(np.abs(x).max()))
        g["logits"] = []
        for toks, n_past in SEQS:
            st.decode(toks, n_past, 8)
            lg = st.get_logits_last(len(toks))
            g["logits"].append(dict(tokens=toks, n_past=n_past, sha256=digest(lg), absmax=float(np.abs(lg).max()), top=int(np.argmax(lg))))
        st.free()
        g["full"] = {}
        for tag, kw in FULL.items():
            for aseed in (0, 1):
                st = ctx.create_state()
                kk = {k: v for k, v in kw.items() if k != "strategy"}
                st.full(W.FullParams(ref, kw.get("strategy", 0), n_threads=8, **kk), wsynth.synth_audio(480000, aseed))
                g["full"]["%s_seed%d" % (tag, aseed)] = segs(st)
                distinct = len({i for sg in g["full"]["%s_seed%d" % (tag, aseed)] for i in sg["ids"]})
                assert distinct >= MIN_DISTINCT, "%s %s seed %d: only %d distinct token ids" % (qt, tag, aseed, distinct)
                st.free()
        g["stream"] = stream_run(W, ref, ctx, 8)
        gold[qt] = g
        ctx.free()
        print(qt, "done", {k: len(v) for k, v in g["full"].items()})
    json.dump(gold, open(os.path.join(ROOT, "tests", "golden", "s256_kquant23.json"), "w"), indent=1)

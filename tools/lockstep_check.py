"""A lock-step group beside its members alone, in one fresh process (the backend reads its switches once per process):

    python3 tools/lockstep_check.py MODEL                 four 30 s chunks (synth_audio seeds 0, 1, 50, 51), greedy, through
                                                          whisper_amd_full_batch and then one by one
    python3 tools/lockstep_check.py MODEL --parallel N    synth_audio(960000, 4) through whisper_full_parallel with N processors

MODEL is a shape name of tools/wsynth.py or name:qtype ("s128:q5_1") for the file the reference's quantizer writes from it.
Prints ONE line of JSON: the segments (ids, tids, t0 / t1, text, p and plog as float32) of the group run ("group": one list per chunk) and of
the solo runs ("solo"), or the stitched segments ("parallel"), and how the group decoded: "steps" (passes formed), "rows" (token rows in
them), "one_launch" (passes that were one launch), "served" (passes that delivered their rows).  tests/test_quant_lockstep_gpu.py reads it."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import numpy as np
import wsynth
import whisper_rs as W

SEEDS = (0, 1, 50, 51)
KW = dict(best_of=1, temperature_inc=0.0)


def segs(st):
    return [dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"], tids=s["tids"],
                 p=[float(np.float32(x)) for x in s["p"]], plog=[float(np.float32(x)) for x in s["plog"]]) for s in st.segments()]


def stats(lib, ptr):
    steps, rows = C.c_long(0), C.c_long(0)
    lib.whisper_amd_batch_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
    lib.whisper_amd_batch_stats(ptr, C.byref(steps), C.byref(rows))
    return dict(steps=steps.value, rows=rows.value, one_launch=int(lib.whisper_amd_batch_one_launch(ptr)), served=int(lib.whisper_amd_batch_served(ptr)))


def main(argv):
    name = argv[1]
    lib = W.load_library(os.environ.get("WA_LIB"))
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    mp = wsynth.quant_model_path(*name.split(":")) if ":" in name else wsynth.model_path(name)
    out = dict(model=name)
    if len(argv) > 3 and argv[2] == "--parallel":
        fc = W.WhisperFullContext.new_with_params(mp, W.WhisperContextParameters(lib), lib=lib)
        rc = fc.full_parallel(W.FullParams(lib, 0, **KW), wsynth.synth_audio(960000, 4), int(argv[3]))
        out.update(rc=rc, parallel=[dict(t0=s["t0"], t1=s["t1"], text=s["text"].decode("latin1"), ids=s["ids"]) for s in fc.segments()])
        out.update(stats(lib, fc.ptr))
        fc.free()
    else:
        ctx = W.WhisperContext.new_with_params(mp, W.WhisperContextParameters(lib), lib=lib)
        fp = W.FullParams(lib, 0, **KW)
        pcms = [wsynth.synth_audio(480000, s) for s in SEEDS]
        states = [ctx.create_state() for _ in pcms]
        W.full_batch(ctx, states, fp, pcms)
        out.update(stats(lib, ctx.ptr))
        out["group"] = [segs(st) for st in states]
        for st in states: st.free()
        out["solo"] = []
        for p in pcms:
            st = ctx.create_state(); st.full(fp, p); out["solo"].append(segs(st)); st.free()
        ctx.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv)

"""Host wall time of full() on a 30 s chunk that lies in device memory, with token_timestamps off and on: what the option costs on the
device path (wa_tts.hip: one energy kernel per call, one snap launch per segment) and on the host path (WHISPER_AMD_TTS_HOST=1: the PCM copied
back, 31.2 M additions on one core, the scans on the host).

  solo    one state, full() on the chunk; off and on alternate, `--calls` each after one warm-up call each
  wave    8 chunks on 8 states through whisper_amd_full_batch, likewise

The host switch is read once per process, so each path runs in a child process of its own; the parent starts them one after the other,
`--rounds` times alternating, and prints one JSON line with every round (the spread between rounds of one path is the noise to hold a
difference against).  The cost of the option is on - off of the same process.  Every full() ends in the stream synchronise of its last
decode step or snap read-back, so the wall time covers the device work.  Works on a library without the switch too (the path is then the
library's only one): run it on the parent commit for the "before" column.
usage: python tools/tts_probe.py [--shape small] [--calls 10] [--rounds 2] [--paths device,host]"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
NB = 8


def summary(ms):
    return {"best_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "calls": len(ms)}


def child(shape, calls):
    import wsynth, whisper_rs as W  # noqa: E401
    lib = W.load_library(os.environ.get("WA_LIB"))
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    hip = C.CDLL("libamdhip64.so")
    ctx = W.WhisperContext.new_with_params(wsynth.model_path(shape), W.WhisperContextParameters(lib), lib=lib)
    states = [ctx.create_state() for _ in range(NB)]
    pcm = []
    for i in range(NB):
        x = wsynth.synth_audio(480000, 100 + i)
        d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), C.c_size_t(x.nbytes)) == 0 and hip.hipMemcpy(d, C.c_void_p(x.ctypes.data), C.c_size_t(x.nbytes), 1) == 0
        pcm.append((d.value, len(x)))
    fps = {tag: W.FullParams(lib, 0, best_of=1, temperature_inc=0.0, token_timestamps=on) for tag, on in (("off", False), ("on", True))}
    out = {"solo": {}, "wave": {}}
    for mode, run in (("solo", lambda fp: states[0].full(fp, pcm[0])), ("wave", lambda fp: W.full_batch(ctx, states, fp, pcm))):
        ms = {"off": [], "on": []}
        for it in range(calls + 1):
            for tag, fp in fps.items():
                t0 = time.perf_counter()
                run(fp)
                if it > 0:
                    ms[tag].append(1e3 * (time.perf_counter() - t0))
        out[mode] = {tag: summary(v) for tag, v in ms.items()}
        out[mode]["option_cost_median_ms"] = round(out[mode]["on"]["median_ms"] - out[mode]["off"]["median_ms"], 3)
        segs = [st.segments() for st in (states[:1] if mode == "solo" else states)]
        out[mode]["segments"] = sum(len(s) for s in segs)
        out[mode]["tokens"] = sum(len(g["ids"]) for s in segs for g in s)
    if hasattr(lib, "whisper_amd_tts_stats"):
        out["stats_state0"] = states[0].tts_stats()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="small")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--paths", default="device,host")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.shape, args.calls)
    out = {"shape": args.shape, "chunks_per_wave": NB}
    for r in range(args.rounds):
        for path in args.paths.split(","):
            env = dict(os.environ, WHISPER_AMD_TTS_HOST="1" if path == "host" else "0")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", args.shape, "--calls", str(args.calls)], env=env,
                               capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-3000:])
                sys.exit(p.returncode)
            out["%s_round%d" % (path, r)] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()

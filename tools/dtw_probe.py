"""Host wall time of the DTW post-processing, the device path (wa_dtw.hip) against the host path (wa_dtw_host.cpp), alternating in ONE process.

  product   whisper_full with dtw_token_timestamps on two states of one context, one created with WHISPER_AMD_DTW_HOST=1 and one without: the
            library's own timer around wa_dtw_timestamps' post-processing (whisper_amd_dtw_timings: decoder pass done -> t_dtw placed, the
            stream synchronise included).  medium shape with N_TOP_MOST 2 (32 heads), a window capped at 48 tokens and a whole window (about
            220 tokens), 1500 frames; small shape with its named preset.
  alone     whisper_amd_dtw_path on a synthetic cube of the same shape, where = 1 (upload + kernels + trace copy + backtrace) against where = 0 (the
            host arithmetic on a cube already in host memory: no copy back, so this flatters the host path).

20 calls each after one warm-up call, best and median, printed as one JSON line.
usage: python tools/dtw_probe.py [--calls 20] [--shapes medium,small] [--no-product] [--no-alone]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import numpy as np  # noqa: E402
import dtw_cases, wsynth, whisper_rs as W  # noqa: E402

AHEADS_SMALL = 8      # whisper.h: WHISPER_AHEADS_SMALL


def summary(ms):
    return {"best_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "calls": len(ms)}


def product(lib, shape, ctx_kw, full_kw, calls):
    ctx = W.WhisperContext.new_with_params(wsynth.model_path(shape), W.WhisperContextParameters(lib, **ctx_kw), lib=lib)
    states = {}
    for tag, env in (("device", "0"), ("host", "1")):        # the switch is read when a state is created
        os.environ["WHISPER_AMD_DTW_HOST"] = env
        states[tag] = ctx.create_state()
    os.environ.pop("WHISPER_AMD_DTW_HOST")
    pcm = wsynth.synth_audio(480000, 5)
    fp = W.FullParams(lib, 1 if "beam_size" in full_kw else 0, **full_kw)
    ms, segs = {"device": [], "host": []}, {}
    for it in range(calls + 1):
        for tag, st in states.items():
            t0, n0 = st.dtw_timings()
            st.full(fp, pcm)
            t1, n1 = st.dtw_timings()
            if it > 0 and n1 > n0:
                ms[tag].append((t1 - t0) / 1e3)
            segs[tag] = [(s["ids"], s["t_dtw"]) for s in st.segments()]
    out = {tag: summary(v) for tag, v in ms.items() if v}
    out["tokens"] = sum(len(s[0]) for s in segs["device"])
    out["dtw_calls_per_full"] = (n1 - n0)
    out["same_result"] = segs["device"] == segs["host"]
    out["stats_device_state"], out["stats_host_state"] = states["device"].dtw_stats(), states["host"].dtw_stats()
    for st in states.values():
        st.free()
    ctx.free()
    return out


def alone(lib, st, n_heads, n_tokens, M, calls):
    c = dtw_cases.shaped("probe", 1, n_heads, n_tokens - 3, M, 1500)
    ms = {0: [], 1: []}
    paths = {}
    for it in range(calls + 1):
        for where in (1, 0):
            t0 = time.perf_counter()
            n, tok, tim = st.dtw_path(c["cube"], M, 2, 7, where)
            dt = 1e3 * (time.perf_counter() - t0)
            assert n > 0, n
            if it > 0:
                ms[where].append(dt)
            paths[where] = (n, tok.tobytes(), tim.tobytes())
    return {"device": summary(ms[1]), "host": summary(ms[0]), "same_path": paths[0] == paths[1], "shape": [n_heads, n_tokens, M]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--shapes", default="medium,small")
    ap.add_argument("--no-product", action="store_true")
    ap.add_argument("--no-alone", action="store_true")
    args = ap.parse_args()
    lib = W.load_library(os.environ.get("WA_LIB"))
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    out = {}
    shapes = args.shapes.split(",")
    if not args.no_product:
        if "medium" in shapes:
            kw = dict(beam_size=5, temperature_inc=0.0, language="zh")
            out["product_medium_ntop2_capped48"] = product(lib, "medium", dict(dtw_preset=W.AHEADS_N_TOP_MOST, dtw_n_top=2), dict(kw, max_tokens=48), args.calls)
            out["product_medium_ntop2_full_window"] = product(lib, "medium", dict(dtw_preset=W.AHEADS_N_TOP_MOST, dtw_n_top=2), kw, args.calls)
        if "small" in shapes:
            out["product_small_preset"] = product(lib, "small", dict(dtw_preset=AHEADS_SMALL), dict(best_of=1, temperature_inc=0.0), args.calls)
    if not args.no_alone:
        ctx = W.WhisperContext.new_with_params(wsynth.model_path("s128"), W.WhisperContextParameters(lib), lib=lib)
        st = ctx.create_state()
        out["alone_32h_48tok_1500"] = alone(lib, st, 32, 48, 1500, args.calls)
        out["alone_32h_223tok_1500"] = alone(lib, st, 32, 223, 1500, args.calls)
        out["alone_10h_223tok_1500"] = alone(lib, st, 10, 223, 1500, args.calls)
        st.free(); ctx.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

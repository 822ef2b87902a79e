"""Forced alignment beside transcription, on the same audio and model, in ONE process.

  full      wall time of full() (greedy, temperature_inc = 0) with DTW token timestamps on 30 s of audio: the autoregressive steps, then the
            teacher-forced DTW pass over their result.
  align     wall time of align() of that result's text token ids (as many as one window holds) on the same audio: log-mel, encoder, ONE
            teacher-forced pass with every text row scored on the device, DTW.
  kernel    device time of k_align_score for those rows between two HIP events (whisper_amd_align_timings), and the bytes of logits that
            stayed on the device (whisper_amd_align_stats).
  host      wall time of the host restatement (whisper_amd_align_score, where = 0) on as many rows of random logits ALREADY in host memory:
            what reducing them on the host costs without the copy that would have to come first; and where = 1 on the same rows, which
            includes their upload - the same bytes over the same link in the other direction.

`--calls` runs of each after one warm-up, best and median, one JSON line.  The full() figure needs no new entry point, so the same command
on the parent commit (with --full-only) gives the same number there.
usage: python tools/align_probe.py [--calls 5] [--shape small] [--full-only]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import numpy as np  # noqa: E402
import wsynth, whisper_rs as W  # noqa: E402

AHEADS = {"small": 8, "base": 6, "tiny": 4}      # whisper.h: WHISPER_AHEADS_*; other shapes: the two top-most layers


def summary(ms):
    return {"best_ms": round(min(ms), 3), "median_ms": round(statistics.median(ms), 3), "calls": len(ms)}


def timed(fn, calls):
    ms = []
    for it in range(calls + 1):
        t0 = time.perf_counter()
        r = fn()
        if it > 0:
            ms.append(1e3 * (time.perf_counter() - t0))
    return r, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--shape", default="small")
    ap.add_argument("--full-only", action="store_true")
    args = ap.parse_args()
    lib = W.load_library(os.environ.get("WA_LIB"))
    W.set_log_callback(lib, lambda lvl, txt: sys.stderr.write(txt) if lvl >= 3 else None)
    kw = dict(dtw_preset=AHEADS[args.shape]) if args.shape in AHEADS else dict(dtw_preset=W.AHEADS_N_TOP_MOST, dtw_n_top=2)
    ctx = W.WhisperContext.new_with_params(wsynth.model_path(args.shape), W.WhisperContextParameters(lib, **kw), lib=lib)
    st = ctx.create_state()
    pcm = wsynth.synth_audio(480000, 5)
    fp = W.FullParams(lib, 0, best_of=1, temperature_inc=0.0)
    out = {"shape": args.shape, "n_vocab": ctx.n_vocab()}

    _, ms = timed(lambda: st.full(fp, pcm), args.calls)
    segs = st.segments()
    ids = [i for s in segs for i in s["ids"] if i < ctx.token_eot()]
    out["full_dtw"] = dict(summary(ms), text_tokens=len(ids), segments=len(segs), placed=sum(t >= 0 for s in segs for t in s["t_dtw"]),
                           dtw_stats=st.dtw_stats(), dtw_post_us_and_calls=st.dtw_timings())
    if not args.full_only:
        ids = ids[:ctx.n_text_ctx() - 4]
        al, ms = timed(lambda: st.align(fp, pcm, ids), args.calls)
        calls_ok, rows, kept = st.align_stats()
        out["align"] = dict(summary(ms), text_tokens=len(ids), rows=len(al), placed=sum(a["t_dtw"] >= 0 for a in al),
                            sum_plog=round(float(sum(a["plog"] for a in al[:-1])), 3))
        out["score_kernel"] = {"device_us": st.align_timings()[0], "rows": len(al), "logits_bytes_kept_per_call": kept // max(calls_ok, 1),
                               "bytes_returned_per_call": 24 * len(al)}
        rng = np.random.default_rng(0)
        x = rng.normal(0.0, 3.0, (len(al), ctx.n_vocab())).astype(np.float32)
        tgt = rng.integers(0, ctx.n_vocab(), len(al))
        _, ms0 = timed(lambda: st.align_score(x, tgt, where=0), args.calls)
        _, ms1 = timed(lambda: st.align_score(x, tgt, where=1), args.calls)
        out["host_restatement_rows_in_host_memory"] = summary(ms0)
        out["upload_and_kernel"] = dict(summary(ms1), kernel_device_us=st.align_timings()[0])
    st.free(); ctx.free()
    print(json.dumps(out))


if __name__ == "__main__":
    main()

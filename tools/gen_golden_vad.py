#!/usr/bin/env python3
"""Golden vectors for voice activity detection: the REFERENCE ENGINE itself (oracle/_ref/libwhisper_ref.so) on the seeded synthetic
VAD model and audio of tools/wsynth_vad.py, and whisper_full(vad = true) on the synthetic s128 model.  Run where that library is built;
writes tests/golden/vad.json (data only).

What comes from where:
  probs, segments, full     the reference library through its C API (probabilities as u32 bit patterns).
  front                     SHA-256 (and a few values) of the [n_chunks][512] LSTM gate inputs.  The reference's graph does not expose
                            that tensor; the digests come from the scalar restatement in tests/native/vad_math.cpp, which this script
                            first pins to the reference: run through the product's host recurrence it must give the reference's
                            probabilities bit for bit, for every input below.
  map                       the reference keeps its time-mapping table inside the state.  Recorded from it: the per-segment
                            (orig_start, orig_end, vad_start, vad_end) and the filtered length, which it logs.  The table and the
                            sweep of every centisecond are this script's own integer restatement (map_table / map_time below), which
                            must contain those recorded points; whisper_full's mapped (t0, t1) under "full" exercise the real table.
"""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools")); sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import wsynth  # noqa: E402
import wsynth_vad as V  # noqa: E402
import whisper_rs as W  # noqa: E402

TILE = 8                                                # WA_VAD_TILE; the front-end cases sit on either side of it
N_SHORT = [1, 511, 512, 513]
FRONT_CHUNKS = [1, TILE - 1, TILE, TILE + 1]            # + the whole audio (438)
SR = 16000


def front_n_samples(chunks):
    return chunks * 512 - 37                            # a partial last window in every case


def build_harness(out_dir):
    exe = os.path.join(out_dir, "vad_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-mavx2", "-mf16c", "-ffp-contract=off",
                           os.path.join(ROOT, "tests", "native", "vad_math.cpp"),
                           os.path.join(ROOT, "whisper-rust_amd", "csrc", "wa_vad_host.cpp"), "-o", exe])
    return exe


def run_harness(exe, lines, work):
    script = os.path.join(work, "script.txt")
    with open(script, "w") as f:
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, script], capture_output=True, text=True, check=True)
    return out.stdout.splitlines()


def fmt_params(ps):
    return " ".join(repr(float(np.float32(x))) if isinstance(x, float) else str(x) for x in ps)


# ---- the speech-only audio's time mapping, restated on integers (whisper.cpp:6644-6790, 7882-7921) ----
def cs_to_samples(cs):
    return int((cs / 100.0) * SR + 0.5)


def samples_to_cs(s):
    return int((s / float(SR)) * 100.0 + 0.5)


def map_table(segs, overlap, n_samples):
    overlap_samples = int(np.float32(overlap) * np.float32(SR))
    silence = int(0.1 * SR)
    total = 0
    for i, (s, e) in enumerate(segs):
        end = cs_to_samples(e) + (overlap_samples if i < len(segs) - 1 else 0)
        total += min(end, n_samples - 1) - cs_to_samples(s)
    total += (len(segs) - 1) * silence if len(segs) > 1 else 0
    table, infos, offset = [], [], 0
    for i, (s, e) in enumerate(segs):
        start = min(cs_to_samples(s), n_samples - 1)
        end = min(cs_to_samples(e) + (overlap_samples if i < len(segs) - 1 else 0), n_samples)
        length = end - start
        if length <= 0:
            continue
        v0, v1 = samples_to_cs(offset), samples_to_cs(offset + length)
        infos.append([s, e, v0, v1])
        table += [(v0, s), (v1, e)]
        if v1 - v0 > 100:
            for j in range(1, (v1 - v0) // 20 - 1 + 1):
                t = v0 + j * 20
                if t < v1:
                    table.append((t, s + ((t - v0) * (e - s)) // (v1 - v0)))
        offset += length
        if i < len(segs) - 1:
            table += [(samples_to_cs(offset), e), (samples_to_cs(offset + silence), segs[i + 1][0])]
            offset += silence
    table.sort(key=lambda p: p[0])                      # stable, as std::sort happens to be irrelevant: duplicates are dropped next
    uniq = []
    for p in table:
        if not uniq or uniq[-1][0] != p[0]:
            uniq.append(p)
    return uniq, infos, total


def map_time(t, table):
    if not table:
        return t
    if t <= table[0][0]:
        return table[0][1]
    if t >= table[-1][0]:
        return table[-1][1]
    k = next(i for i, p in enumerate(table) if p[0] >= t)
    if table[k][0] == t:
        return table[k][1]
    lo, up = table[k - 1], table[k]
    return lo[1] + ((t - lo[0]) * (up[1] - lo[1])) // (up[0] - lo[0])


def main():
    ref_path = os.path.join(ROOT, "oracle", "_ref", "libwhisper_ref.so")
    ref = W.load_library(ref_path)
    log = []
    W.set_log_callback(ref, lambda lvl, txt: log.append(txt))
    mp, pcm = V.model_path(), V.synth_audio()
    work = tempfile.mkdtemp(prefix="vad_golden")
    exe = build_harness(work)
    pcm_path = os.path.join(work, "audio.f32")
    pcm.tofile(pcm_path)
    u32 = lambda a: [int(x) for x in np.asarray(a, dtype=np.float32).view(np.uint32)]

    golden = dict(tile=TILE, n_samples=len(pcm),
                  model_sha256=hashlib.sha256(open(mp, "rb").read()).hexdigest(), audio_sha256=hashlib.sha256(pcm.tobytes()).hexdigest())

    # probabilities: the reference, and the harness pinned to it
    v = W.WhisperVadContext.new(mp, lib=ref)
    cases = {"full": len(pcm)}
    cases.update({"n%d" % n: n for n in N_SHORT})
    cases.update({"c%d" % c: front_n_samples(c) for c in FRONT_CHUNKS})
    golden["probs"] = {}
    for tag, n in cases.items():
        golden["probs"][tag] = dict(n_samples=n, bits=u32(v.detect_speech(pcm[:n])))
    again = u32(v.detect_speech(pcm))                   # the LSTM state is reset by every call
    assert again == golden["probs"]["full"]["bits"]
    out = run_harness(exe, ["model " + mp, "audio " + pcm_path] + ["probs %d" % n for n in cases.values()], work)
    assert out[0] == "model ok", out[0]
    for (tag, n), line in zip(cases.items(), out[2:]):
        got = [int(x, 16) for x in line.split()[2:]]
        assert got == golden["probs"][tag]["bits"], "the scalar restatement differs from the reference for %s" % tag
    p = np.array(golden["probs"]["full"]["bits"], dtype=np.uint32).view(np.float32)
    print("probs: %d in [%.3f, %.3f], %d >= 0.5, %d < 0.35" % (len(p), p.min(), p.max(), (p >= 0.5).sum(), (p < 0.35).sum()))

    # front-end digests (harness, now pinned)
    golden["front"] = {}
    front_cases = {"c%d" % c: front_n_samples(c) for c in FRONT_CHUNKS}
    front_cases["full"] = len(pcm)
    for tag, n in front_cases.items():
        path = os.path.join(work, "front_%s.f32" % tag)
        assert run_harness(exe, ["model " + mp, "audio " + pcm_path, "front %d %s" % (n, path)], work)[-1].startswith("front ")
        g = np.fromfile(path, dtype=np.float32).reshape(-1, 512)
        rows = sorted({0, len(g) // 2, len(g) - 1})
        golden["front"][tag] = dict(n_samples=n, n_chunks=len(g), sha256=hashlib.sha256(g.tobytes()).hexdigest(),
                                    rows={str(r): u32(g[r, ::64]) for r in rows})

    # segments for the three parameter sets
    golden["segments"], golden["map"] = {}, {}
    v.detect_speech(pcm)
    for tag, ps in V.PARAM_SETS.items():
        segs = v.segments_from_probs(W.vad_params(ref, *ps))
        assert segs == v.segments_from_samples(W.vad_params(ref, *ps), pcm)
        golden["segments"][tag] = dict(params=[float(np.float32(x)) if isinstance(x, float) else x for x in ps], segments=[[int(a), int(b)] for a, b in segs])
    assert len(golden["segments"]["default"]["segments"]) >= 2
    for tag in ("max1.5s", "thr0.6"):
        assert golden["segments"][tag]["segments"] != golden["segments"]["default"]["segments"], tag
    v.free()

    # whisper_full(vad = true) on s128, and the reference's own record of its mapping (from its log)
    wp = wsynth.model_path("s128")
    golden["full"] = {}

    def full_ctx():
        return W.WhisperFullContext.new_with_params(wp, W.WhisperContextParameters(ref, use_gpu=False), lib=ref)

    def params(**kw):
        fp = W.FullParams(ref, best_of=1, temperature_inc=0.0, n_threads=8, vad=True, vad_model_path=mp, **kw)
        return fp

    def take(ctx):
        return [dict(t0=s["t0"], t1=s["t1"], ids=s["ids"], tok_t0=s["tok_t0"], tok_t1=s["tok_t1"]) for s in ctx.segments()]

    for tag, ps in V.PARAM_SETS.items():
        del log[:]
        ctx = full_ctx()
        fp = params()
        fp.set("vad_params", W.vad_params(ref, *ps))
        assert ctx.full(fp, pcm) == 0
        golden["full"]["greedy_" + tag] = take(ctx)
        text = "".join(log)
        infos = [[int(round(float(x) * 100)) for x in m] for m in
                 re.findall(r"vad_segment_info: orig_start: ([\d.]+), orig_end: ([\d.]+), vad_start: ([\d.]+), vad_end: ([\d.]+)", text)]
        n_filtered = int(re.search(r"Reduced audio from \d+ to (\d+) samples", text).group(1))
        segs = [tuple(s) for s in golden["segments"][tag]["segments"]]
        table, my_infos, total = map_table(segs, ps[5], len(pcm))
        assert infos == my_infos, (infos, my_infos)
        for o0, o1, v0, v1 in infos:
            assert (v0, o0) in table or any(t[0] == v0 for t in table)
        m = total * 100 // SR + 2
        golden["map"][tag] = dict(ref_segment_info=infos, ref_n_copied=n_filtered, n_filtered=total, table=[list(t) for t in table],
                                  sweep=[map_time(t, table) for t in range(m)])
        if tag == "default":
            # as in the reference, a later vad = false call on the same context still maps its times through the last table
            fp2 = W.FullParams(ref, best_of=1, temperature_inc=0.0, n_threads=8)
            assert ctx.full(fp2, pcm[:SR * 6]) == 0
            golden["full"]["then_vad_off_6s"] = take(ctx)
        ctx.free()
    assert golden["full"]["greedy_default"] and golden["full"]["greedy_default"][0]["t0"] != 0

    ctx = full_ctx()
    assert ctx.full(params(token_timestamps=True), pcm) == 0
    golden["full"]["greedy_token_timestamps"] = take(ctx)
    assert ctx.full(params(), np.zeros(3 * SR, dtype=np.float32)) == 0          # no speech: 0, results cleared
    assert ctx.segments() == []
    ctx.free()
    ctx = full_ctx()
    assert ctx.full_parallel(params(), pcm, 2) == 0
    golden["full"]["parallel2"] = take(ctx)
    ctx.free()
    ctx = full_ctx()
    assert ctx.full(W.FullParams(ref, best_of=1, temperature_inc=0.0, n_threads=8), pcm) == 0
    golden["full"]["vad_off"] = take(ctx)
    ctx.free()

    out_path = os.path.join(ROOT, "tests", "golden", "vad.json")
    with open(out_path, "w") as f:
        json.dump(golden, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", out_path, os.path.getsize(out_path), "bytes;", {k: (len(s), sum(len(x["ids"]) for x in s)) for k, s in golden["full"].items()})


if __name__ == "__main__":
    main()

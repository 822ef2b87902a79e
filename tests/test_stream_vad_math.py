"""The incremental speech segmenter of live VAD sessions (whisper-rust_amd/csrc/wa_stream_vad.h through tests/native/stream_vad_plan.cpp, g++
alone: no HIP, no device) against the offline rules: wa_vad_segments_from_probs in the same program, and tools/stream_vad_ref.py.

1. Fed window by window and flushed, the segmenter gives the offline list: built sequences - neighbours 3072 and 3584 samples apart (the first
   pass only makes multiples of 512), a candidate inside the gap that min_speech discards and one that lives on, speech running to the end,
   max_speech hit with and without a prev_end, a first speech closer to 0 than the pad - and seeded random ones, each with speech_pad_ms 0, 30
   and 100 and several other settings.
2. A gap of exactly 3199 samples merges and one of exactly 3200 does not: speeches handed to the merge stage directly, against the restatement.
3. What is handed out before the flush is final: it comes out at the window the restatement names, within wa_svad_delay_bound where no
   candidate opens behind it, and the offline list of the same probabilities followed by ANY other tail starts with it.
4. The split at the length cap equals the restatement (tools/stream_vad_ref.py: capped), flags and ranges; no utterance is longer than the cap.
5. Deliberately wrong variants each change an expected list: the merge look-ahead one window short, padding decided before the merge, <= for <
   at 3200.
6. What open refuses (wa_svad_params_ok).
7. The driver built with -fsanitize=address,undefined runs clean as a stand-alone program and prints the same.
8. The code object wa_vad_k.o holds k_vad_front and k_stream_vad_front and neither has scratch or a spilled register.
CPU only."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stream_vad_ref as R  # noqa: E402

SRC = [os.path.join(ROOT, "tests", "native", "stream_vad_plan.cpp"), os.path.join(ROOT, "whisper-rust_amd", "csrc", "wa_vad_host.cpp")]
INC = "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc")
FLAGS = ["-std=c++17", "-ffp-contract=off", "-mavx2", "-mf16c", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function"]

HI, LO, MID = 0.9, 0.05, 0.42          # at or above the threshold, below the negative threshold (0.35), between the two


def seq(*runs):
    return np.concatenate([np.full(n, p, np.float32) for n, p in runs])


BUILT = {
    # 10 windows of speech, 6 of silence (3072 < 3200: merged), 10 of speech, 7 of silence (3584: not merged), 10 of speech
    "gaps_3072_3584": seq((3, LO), (10, HI), (6, LO), (10, HI), (7, LO), (10, HI), (20, LO)),
    # one window of speech 512 behind the first end: discarded by min_speech at the window 3072 behind that end
    "candidate_discarded": seq((2, LO), (10, HI), (1, LO), (1, HI), (12, LO), (10, HI), (12, LO)),
    # the same candidate, but the window that would discard it is speech again: the candidate lives on and is merged
    "candidate_lives": seq((2, LO), (10, HI), (1, LO), (1, HI), (4, LO), (12, HI), (12, LO)),
    # probabilities between the thresholds keep a speech open: nothing is decided before they fall
    "hovering": seq((2, LO), (10, HI), (30, MID), (8, LO), (10, HI), (9, LO)),
    "speech_to_the_end": seq((4, LO), (10, HI), (9, LO), (15, HI)),
    "speech_from_zero": seq((12, HI), (20, LO), (9, HI), (3, LO)),
    "speech_from_1024": seq((2, LO), (12, HI), (20, LO)),
    "silence": seq((40, LO)),
    "short_only": seq((5, LO), (3, HI), (30, LO)),
}
# max_speech_duration_s = 2: max_speech_samples = 32000 - 512 - 2 pad.  min_silence 300 ms lets a dip of 5 windows set prev_end without ending
# the speech
LONG = {
    "max_speech_no_prev_end": seq((2, LO), (150, HI), (12, LO)),
    "max_speech_prev_end": seq((2, LO), (30, HI), (5, LO), (40, HI), (5, LO), (60, HI), (14, LO)),
    "max_speech_prev_end_then_silence": seq((2, LO), (52, HI), (12, LO), (30, HI), (14, LO)),
}
SETTINGS = [dict(speech_pad_ms=0), dict(speech_pad_ms=30), dict(speech_pad_ms=100), dict(speech_pad_ms=30, min_silence_duration_ms=0, min_speech_duration_ms=0),
            dict(speech_pad_ms=100, min_silence_duration_ms=500, min_speech_duration_ms=100, threshold=0.6)]
LONG_SETTINGS = [dict(max_speech_duration_s=2.0, min_silence_duration_ms=300, speech_pad_ms=pad) for pad in (0, 30, 100)]


def random_probs(rng, n):
    out = []
    while len(out) < n:
        kind = rng.integers(0, 5)
        run = int(rng.integers(1, 14))
        out += {0: [LO] * run, 1: [HI] * run, 2: [MID] * run, 3: list(rng.uniform(0.0, 1.0, run)), 4: [HI, LO] * (run // 2 + 1)}[int(kind)]
    return np.asarray(out[:n], np.float32)


def line_of(cmd, params, cap_ms, var, path):
    p = dict(R.DEFAULTS, **params)
    return "%s %r %d %d %r %d %d %d %s" % (cmd, float(np.float32(p["threshold"])), p["min_speech_duration_ms"], p["min_silence_duration_ms"],
                                          float(np.float32(p["max_speech_duration_s"])), p["speech_pad_ms"], cap_ms, var, path)


def parse(lines, at, with_off=True):
    out = {}
    if with_off:
        out["ok"] = lines[at].split()[1] == "ok"; at += 1
    tag, k, splits = lines[at].split(); at += 1
    assert tag == "inc"
    rows = [[int(v) for v in lines[at + i].split()] for i in range(int(k))]; at += int(k)
    out.update(inc=[(r[0], r[1]) for r in rows], split=[r[2] for r in rows], raw_end=[r[3] for r in rows], win=[r[4] for r in rows], length=[r[5] for r in rows],
               splits=int(splits))
    if with_off:
        tag, m = lines[at].split(); at += 1
        assert tag == "off"
        out["off"] = [tuple(int(v) for v in lines[at + i].split()) for i in range(int(m))]; at += int(m)
        tag, b = lines[at].split(); at += 1
        assert tag == "bound"
        out["bound"] = int(b)
    return out, at


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    work = tmp_path_factory.mktemp("stream_vad")
    exe = str(work / "stream_vad_plan")
    subprocess.check_call(["g++", "-O2"] + FLAGS + [INC] + SRC + ["-o", exe])
    rng = np.random.default_rng(20261021)
    cases = []              # (name, probs, params, cap_ms, var)
    for name, probs in BUILT.items():
        cases += [(name, probs, s, 30000, v) for s in SETTINGS for v in (0, 1, 2, 3)]
    for name, probs in LONG.items():
        cases += [(name, probs, s, 30000, 0) for s in LONG_SETTINGS]
        cases += [(name, probs, s, 2000, 0) for s in LONG_SETTINGS] + [(name, probs, s, 3000, 0) for s in LONG_SETTINGS]
    for k in range(24):
        probs = random_probs(rng, int(rng.integers(40, 400)))
        cases += [("random%d" % k, probs, SETTINGS[k % len(SETTINGS)], 30000, 0)]
        cases += [("random%d" % k, probs, dict(LONG_SETTINGS[k % 3], max_speech_duration_s=1.0), 30000, 0)]
        cases += [("random%d" % k, probs, dict(LONG_SETTINGS[k % 3], max_speech_duration_s=1.0), 1500, 0)]
    lines = []
    for n, (name, probs, params, cap, var) in enumerate(cases):
        path = str(work / ("probs_%d.f32" % n))
        probs.tofile(path)
        lines.append(line_of("run", params, cap, var, path))
    cmd = str(work / "cmd.txt")
    open(cmd, "w").write("".join(l + "\n" for l in lines))
    r = subprocess.run([exe, cmd], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    out, at, res = r.stdout.splitlines(), 0, []
    for c in cases:
        got, at = parse(out, at)
        res.append((c, got))
    assert at == len(out)
    return dict(exe=exe, work=work, cmd=cmd, stdout=r.stdout, res=res, rng=rng)


def right(env):
    return [(c, g) for c, g in env["res"] if c[4] == 0]


def test_incremental_list_is_the_offline_list(env):
    n_segments = merged = 0
    for (name, probs, params, cap, _), g in right(env):
        assert g["off"] == R.segments(probs, params), ("the restatement against wa_vad_segments_from_probs", name, params)
        if g["splits"] == 0:
            assert g["inc"] == g["off"], (name, params, cap)
            n_segments += len(g["inc"])
    assert n_segments > 200
    by = {(c[0], c[2]["speech_pad_ms"]): g for c, g in right(env) if c[3] == 30000 and c[2] in SETTINGS[:3]}
    for pad in (0, 30, 100):
        assert len(by[("gaps_3072_3584", pad)]["inc"]) == 2 and len(by[("candidate_discarded", pad)]["inc"]) == 2
        assert len(by[("candidate_lives", pad)]["inc"]) == 1 and len(by[("speech_to_the_end", pad)]["inc"]) == 2
        assert by[("speech_from_zero", pad)]["inc"][0][0] == 0 and by[("silence", pad)]["inc"] == [] and by[("short_only", pad)]["inc"] == []
        assert by[("speech_to_the_end", pad)]["win"][-1] == -1
    assert by[("speech_from_1024", 100)]["inc"][0][0] == 0 and by[("speech_from_1024", 30)]["inc"][0][0] == R.samples_to_cs(1024 - 480)
    longs = {c[0]: g for c, g in right(env) if c[0] in LONG and c[3] == 30000 and c[2]["speech_pad_ms"] == 30}
    for name, g in longs.items():           # max_speech was hit: the first pass pushed more speeches than the list holds
        raw = R.first_pass(LONG[name], R.constants(LONG_SETTINGS[1]))[0]
        cut = [r for r in raw if r[2] is not None and LONG[name][r[2]] >= 0.5 or r[2] is not None and r[1] < 512 * (r[2] - 9)]
        assert len(cut) >= 1 and g["splits"] == 0, (name, raw)          # max_speech cut a speech: pushed by a speech window, or well behind its end
        merged += len(raw) > len(g["off"])
    assert merged == 2 and len(longs) == 3


def test_gap_of_3199_and_3200(env):
    """the merge stage on speeches handed to it directly"""
    lines, want = [], []
    for gap in (3199, 3200, 3201):
        for pad in (0, 30, 100):
            raws = [(5000, 15000), (15000 + gap, 30000), (40000, 50000)]
            params = dict(speech_pad_ms=pad)
            path = str(env["work"] / ("raws_%d_%d.i32" % (gap, pad)))
            np.asarray([100] + [v for r in raws for v in r], np.int32).tofile(path)
            for var in (0, 3):
                lines.append(line_of("raws", params, 30000, var, path))
            want.append((gap, R.finish(raws, R.constants(params), 100 * 512)))
    cmd = str(env["work"] / "cmd_raws.txt")
    open(cmd, "w").write("".join(l + "\n" for l in lines))
    r = subprocess.run([env["exe"], cmd], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    out, at = r.stdout.splitlines(), 0
    for gap, w in want:
        got, at = parse(out, at, with_off=False)
        le, at = parse(out, at, with_off=False)
        assert got["inc"] == w and len(w) == (2 if gap < 3200 else 3), gap
        assert (le["inc"] != w) == (gap == 3200), ("<= for < shows at 3200 and only there", gap)


def test_handed_out_early_is_final_and_in_time(env):
    rng = np.random.default_rng(7)
    early = in_bound = 0
    for (name, probs, params, cap, _), g in right(env):
        if g["splits"] != 0:
            continue
        want = R.emit_windows(probs, params)
        assert [(-1 if w is None else w, e) for w, e in want] == list(zip(g["win"], g["raw_end"])), (name, params)
        c = R.constants(params)
        for k, (w, e) in enumerate(zip(g["win"], g["raw_end"])):
            if w < 0:
                continue
            early += 1
            behind = probs[e // 512:w + 1]
            if np.all(behind < c["neg"]):                   # no candidate, nothing hovering: the stated bound holds
                assert 512 * (w + 1) - e <= g["bound"], (name, params, k)
                in_bound += 1
            for _ in range(3):                              # later audio cannot change it
                alt = np.concatenate([probs[:w + 1], random_probs(rng, 60)])
                assert R.segments(alt, params)[:k + 1] == g["inc"][:k + 1], (name, params, k)
    assert early > 100 and in_bound > 50
    assert R.constants(R.DEFAULTS)["min_silence"] == 1600 and [g["bound"] for c, g in right(env) if c[2] == SETTINGS[1]][0] == 3584
    assert [g["bound"] for c, g in right(env) if c[2] == SETTINGS[4]][0] == 8192 + 512


def test_split_at_the_cap_is_the_restatement(env):
    n_split = 0
    for (name, probs, params, cap, _), g in right(env):
        want, splits = R.capped(probs, params, cap)
        assert g["ok"], (name, params, cap)
        assert (g["inc"], g["split"], g["splits"]) == ([(a, b) for a, b, _ in want], [1 if s else 0 for _, _, s in want], splits), (name, params, cap)
        T = 512 * len(probs)
        assert g["length"] == [R.utterance_range(s, T)[1] for s in g["inc"]]
        assert all(0 < n <= cap * 16 for n in g["length"]), (name, params, cap, g["length"])
        n_split += splits
        if splits == 0:
            assert [(a, b) for a, b, _ in want] == R.segments(probs, params)
    assert n_split > 30
    capped = {(c[0], c[3]): g for c, g in right(env) if c[0] in LONG and c[2]["speech_pad_ms"] == 30}
    assert capped[("max_speech_no_prev_end", 2000)]["splits"] >= 2 and capped[("max_speech_prev_end", 2000)]["splits"] >= 1


def test_wrong_variants_change_a_list(env):
    changed = {1: [], 2: [], 3: []}
    rights = {(c[0], id(c[2])): g for c, g in env["res"] if c[4] == 0 and c[3] == 30000}
    for (name, probs, params, cap, var), g in env["res"]:
        if var and g["inc"] != rights[(name, id(params))]["inc"]:
            changed[var].append(name)
    assert "gaps_3072_3584" in changed[1] and "gaps_3072_3584" in changed[2], changed
    # <= for < needs a gap of exactly 3200, which the first pass cannot make: test_gap_of_3199_and_3200 shows that one
    assert changed[3] == []


def test_open_refusals(env):
    lines = []
    sets = [(dict(), 30000, True), (dict(speech_pad_ms=101), 30000, False), (dict(speech_pad_ms=100), 30000, True), (dict(), 0, False), (dict(), 30001, False),
            (dict(max_speech_duration_s=30.5), 30000, False), (dict(max_speech_duration_s=10.0), 9999, False), (dict(max_speech_duration_s=10.0), 10000, True),
            (dict(max_speech_duration_s=1e9), 30000, False), (dict(max_speech_duration_s=0.0), 30000, False), (dict(speech_pad_ms=-1), 30000, False)]
    path = str(env["work"] / "probs_refusals.f32")
    BUILT["silence"].tofile(path)
    for params, cap, _ in sets:
        lines.append(line_of("run", params, cap, 0, path))
    cmd = str(env["work"] / "cmd_refusals.txt")
    open(cmd, "w").write("".join(l + "\n" for l in lines))
    r = subprocess.run([env["exe"], cmd], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [l.split()[1] == "ok" for l in r.stdout.splitlines() if l.startswith("params")]
    assert got == [ok for _, _, ok in sets]


def test_sanitized_driver_prints_the_same(env):
    exe = str(env["work"] / "stream_vad_plan_san")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] + FLAGS + [INC] + SRC + ["-o", exe])
    r = subprocess.run([exe, env["cmd"]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout == env["stdout"]


def test_no_scratch_no_spills(tmp_path):
    """wa_vad_k.o: k_vad_front and k_stream_vad_front have no scratch and no spilled register (the check of tests/test_kquant_math.py)"""
    tools = "/opt/rocm/lib/llvm/bin"
    obj = os.path.join(ROOT, "whisper-rust_amd", "build", "wa_vad_k.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(tools, "clang-offload-bundler")):
        pytest.skip("no build tree / LLVM tools here")
    fat, co = str(tmp_path / "fat"), str(tmp_path / "co")
    subprocess.check_call([os.path.join(tools, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(tools, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    notes = subprocess.check_output([os.path.join(tools, "llvm-readelf"), "--notes", co], text=True)
    seen, name = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith(".name:"):
            name = line.split(":", 1)[1].strip()
        elif name and (line.startswith(".private_segment_fixed_size:") or line.startswith(".vgpr_spill_count:") or line.startswith(".sgpr_spill_count:")):
            seen.setdefault(name, {})[line.split(":")[0]] = int(line.split(":")[1])
    assert any("k_stream_vad_front" in k for k in seen) and any("k_vad_front" in k for k in seen), sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

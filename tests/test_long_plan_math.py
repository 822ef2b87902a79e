"""The chunk planner of whisper_amd_full_long (whisper-rust_amd/csrc/wa_long_plan.h through tests/native/long_plan.cpp, g++ alone: no HIP,
no device).

A long recording is cut into chunks of whole VAD segments, greedy and in order, each at most `cap` samples of speech-only audio unless it
is a single segment.  The packed length and time table of a chunk are by definition what wa_vad_filter_audio computes for that run of
segments taken as the whole list; the driver prints both statements (wa_vad_layout_make, which the planner and the device pack use, and
wa_vad_filter_audio over a ramp signal) and they must agree, chunk by chunk and for the whole list, where the whole list must also give the
table recorded from the reference engine (tests/golden/vad.json).  The plans are compared to a numpy restatement of the planner written in this
file, and tools/long_ref.py - the restatement the GPU tests share - is held to it too.  The same driver built with -fsanitize=address,undefined runs clean as a stand-alone program.  CPU only."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import long_ref as R
import wsynth_vad as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = json.load(open(os.path.join(ROOT, "tests", "golden", "vad.json")))
SRCS = [os.path.join(ROOT, "tests", "native", "long_plan.cpp"), os.path.join(ROOT, "whisper-rust_amd", "csrc", "wa_vad_host.cpp")]
N = G["n_samples"]                  # 14 s + 137 samples
OV = 0.1

# cap (ms) -> chunks (first, count, packed samples) for the `default` segments [[103,224],[704,953],[1203,1264]]
TABLE = {
    30000: [(0, 3, 75360)],
    4000:  [(0, 2, 62400), (2, 1, 9760)],
    3500:  [(0, 1, 19360), (1, 2, 52800)],
    3000:  [(0, 1, 19360), (1, 1, 39840), (2, 1, 9760)],
    1000:  [(0, 1, 19360), (1, 1, 39840), (2, 1, 9760)],           # every segment is longer than the cap
}


# ---- the planner restated here, in numpy, from the issue's rule and the reference's VAD step (whisper.cpp:6644-6676); the driver's plans are held
# ---- to THIS; tools/long_ref.py, which the GPU tests share, is held to it as well (test_shared_restatement_agrees) ----
def length_restated(segs, overlap, n_samples):
    """samples of speech-only audio of `segs` taken as the whole list: every segment's end + overlap except the last one's, ends clamped to
    n_samples - 1, 0.1 s of silence per gap, never negative"""
    if len(segs) == 0:
        return 0
    s = np.asarray(segs, dtype=np.float64)
    start = np.floor(s[:, 0] / 100.0 * 16000 + 0.5).astype(np.int64)
    end = np.floor(s[:, 1] / 100.0 * 16000 + 0.5).astype(np.int64)
    end[:-1] += int(np.float32(overlap) * np.float32(16000))
    return max(int((np.minimum(end, n_samples - 1) - start).sum()) + (len(segs) - 1) * 1600, 0)


def plan_restated(segs, n_samples, overlap, cap):
    out, first = [], 0
    while first < len(segs):
        count = 1
        while first + count < len(segs) and length_restated(segs[first:first + count + 1], overlap, n_samples) <= cap:
            count += 1
        out.append((first, count, length_restated(segs[first:first + count], overlap, n_samples)))
        first += count
    return out


def segs_of(tag):
    return [tuple(s) for s in G["segments"][tag]["segments"]]


def fmt_case(n_samples, overlap, cap, segs):
    return "%d %r %d %d %s" % (n_samples, float(np.float32(overlap)), cap, len(segs), " ".join("%d %d" % s for s in segs))


def parse_lt(f):
    """'L <len> <n> p o ... F <len> <n> p o ...' -> ((len, table), (len, table))"""
    out, at = [], 0
    for tag in ("L", "F"):
        assert f[at] == tag
        length, n = int(f[at + 1]), int(f[at + 2])
        out.append((length, [(int(f[at + 3 + 2 * i]), int(f[at + 4 + 2 * i])) for i in range(n)]))
        at += 3 + 2 * n
    assert at == len(f)
    return out


def run_driver(exe, work, cases, tag):
    inp = str(work / ("cases_%s.txt" % tag))
    with open(inp, "w") as f:
        f.write("\n".join(fmt_case(*c) for c in cases) + "\n")
    r = subprocess.run([exe, inp], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    lines, at, res = r.stdout.split("\n"), 0, []
    for _ in cases:
        head = lines[at].split(); at += 1
        assert head[0] == "plan"
        chunks = []
        for _ in range(int(head[1])):
            f = lines[at].split(); at += 1
            assert f[0] == "chunk"
            chunks.append(((int(f[1]), int(f[2]), int(f[3])),) + tuple(parse_lt(f[4:])))
        f = lines[at].split(); at += 1
        assert f[0] == "whole"
        whole = parse_lt(f[1:])
        assert lines[at].split() == ["pieces", "1"], "the pieces of wa_vad_layout_make do not rebuild wa_vad_filter_audio's audio"; at += 1
        res.append(dict(chunks=chunks, whole=whole))
    return res


def random_cases(seed=20240611, n=200):
    rng, cases = np.random.default_rng(seed), []
    for _ in range(n):
        k = int(rng.integers(1, 41))
        lens = np.exp(rng.uniform(np.log(1.0), np.log(4000.0), k)).astype(np.int64).clip(1, 4000)        # 1 cs .. 40 s
        gaps = rng.integers(0, 300, k)
        segs, t = [], int(rng.integers(0, 200))
        for ln, gp in zip(lens, gaps):
            segs.append((t, t + int(ln)))
            t += int(ln) + int(gp)                       # gap 0: back-to-back segments
        end = R.cs_to_samples(segs[-1][1])
        mode = int(rng.integers(0, 4))                   # the audio ends beyond, at, one short of, or well inside the last segment(s)
        n_samples = end + int(rng.integers(1, 5000)) if mode == 0 else end if mode == 1 else max(end - 1, 2) if mode == 2 else max(end - int(rng.integers(2, 40000)), 2)
        cap = int(rng.choice([16000, 48000, 160000, 480000]))
        cases.append((n_samples, OV if rng.integers(0, 4) else 0.0, cap, segs))
    return cases


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    work = tmp_path_factory.mktemp("long_plan")
    exe = str(work / "long_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-mavx2", "-mf16c", "-ffp-contract=off"] + SRCS + ["-o", exe])
    return dict(work=work, exe=exe)


def test_header_compiles_alone(env):
    """wa_long_plan.h with g++ and nothing else of the product but wa_vad.h's declarations."""
    src = env["work"] / "alone.cpp"
    src.write_text('#include "wa_long_plan.h"\nint main() { wa_vad_seg s = { 103, 224 }; return wa_long_plan(&s, 1, 224137, 0.1f, 480000).size() == 1 ? 0 : 1; }\n')
    exe = str(env["work"] / "alone")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc"), str(src), "-o", exe])
    assert subprocess.run([exe]).returncode == 0


@pytest.fixture(scope="module")
def golden_runs(env):
    cases = [(N, OV, ms * 16, segs_of("default")) for ms in TABLE]
    cases += [(N, OV, ms * 16, segs_of(t)) for t in ("max1.5s", "thr0.6") for ms in TABLE]
    return cases, run_driver(env["exe"], env["work"], cases, "golden")


def test_golden_segments_table(golden_runs):
    cases, res = golden_runs
    for (_, _, cap, _), r, want in zip(cases, res, TABLE.values()):
        assert [c[0] for c in r["chunks"]] == want, "cap %d samples" % cap


def test_other_golden_segment_lists(golden_runs):
    cases, res = golden_runs
    assert len(cases) == 3 * len(TABLE)
    for (n, ov, cap, segs), r in list(zip(cases, res))[len(TABLE):]:
        assert [c[0] for c in r["chunks"]] == plan_restated(segs, n, ov, cap)


def test_whole_list_equals_the_recorded_mapping(golden_runs):
    cases, res = golden_runs
    for i, tag in ((0, "default"), (len(TABLE), "max1.5s"), (2 * len(TABLE), "thr0.6")):
        (ll, lt), (fl, ft) = res[i]["whole"]
        assert ll == fl == G["map"][tag]["n_filtered"]
        assert lt == ft == [tuple(p) for p in G["map"][tag]["table"]]
        assert ll == length_restated(cases[i][3], OV, N) and lt == R.layout(cases[i][3], OV, N)[2]


def check_case(case, r):
    n, ov, cap, segs = case
    plan = [c[0] for c in r["chunks"]]
    assert plan == plan_restated(segs, n, ov, cap)
    at = 0
    for (first, count, packed), (ll, lt), (fl, ft) in r["chunks"]:
        assert first == at and count >= 1                                      # the chunks partition the segments in order
        at += count
        assert packed == ll == fl == length_restated(segs[first:first + count], ov, n)       # ... with the length wa_vad_filter_audio gives the sub-list
        assert lt == ft                                                        # ... and its table
        assert packed <= cap or count == 1                                     # at most the cap unless a single segment
        if at < len(segs):                                                     # the next segment would not have fitted
            assert length_restated(segs[first:first + count + 1], ov, n) > cap
    assert at == len(segs)
    (ll, lt), (fl, ft) = r["whole"]
    assert ll == fl and lt == ft


def test_seeded_random_lists(env):
    cases = random_cases()
    res = run_driver(env["exe"], env["work"], cases, "random")
    assert len(res) == len(cases) == 200
    for case, r in zip(cases, res):
        check_case(case, r)
    counts = [len(r["chunks"]) for r in res]
    assert max(counts) > 5 and min(counts) == 1                               # the cases do cut, and do not always
    assert any(c[0][1] == 1 and c[0][2] > case[2] for case, r in zip(cases, res) for c in r["chunks"])       # a single segment over the cap occurs
    assert any(R.cs_to_samples(case[3][-1][1]) >= case[0] for case in cases)                                 # ends at or beyond n_samples occur


def test_shared_restatement_agrees():
    """tools/long_ref.py - what the GPU tests plan and measure lengths with - against the restatement written in this file, on the random lists
    and the golden ones: an error in the shared module would not be shared by this file."""
    cases = random_cases() + [(N, OV, ms * 16, segs_of(t)) for t in V.PARAM_SETS for ms in TABLE]
    for n, ov, cap, segs in cases:
        assert R.plan(segs, n, ov, cap) == plan_restated(segs, n, ov, cap)
        assert R.layout_length(segs, ov, n) == length_restated(segs, ov, n) == R.layout(segs, ov, n)[0]


def test_restatement_agrees_on_tables_of_the_golden_chunks(golden_runs):
    """tools/long_ref.py's table - the one the GPU tests map times with - against the product's, for every chunk of every golden plan."""
    cases, res = golden_runs
    for (n, ov, _, segs), r in zip(cases, res):
        for (first, count, packed), (ll, lt), _ in r["chunks"]:
            total, _, table = R.layout(segs[first:first + count], ov, n)
            assert (total, table) == (ll, lt)


def test_driver_under_sanitizers(env):
    """The driver as a stand-alone program with AddressSanitizer and UBSan: the random cases, no report."""
    exe = str(env["work"] / "long_plan_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-mavx2", "-mf16c",
                           "-ffp-contract=off"] + SRCS + ["-o", exe])
    cases = random_cases(n=60)
    res = run_driver(exe, env["work"], cases, "san")
    for case, r in zip(cases, res):
        check_case(case, r)

"""The streaming sessions' host code (whisper-rust_amd/csrc/wa_stream.h through tests/native/stream_plan.cpp, g++ alone: no HIP, no device).

1. The session plan against the literal vectors of tools/stream_ref.py (the reference's examples/stream/stream.cpp, step mode) over 14 windows
   of eight (step, length, keep) triples - keep > step, length < step, length == step and a non-integer length / step among them: n_new_line,
   take, length and commit flag of every window, and every window is the range [e - len, e), e = (k + 1) n_step, len <= n_keep + n_len, of
   the session's sample axis (the audio is its own index, so a window's content names its range).
2. The drop rule: 2 n_step pending samples drop nothing, 2 n_step + 1 drop all of them and run no window; the next window is two ranges.
3. Ring pieces of ranges that end on the last slot, start at slot 0, or wrap.
4. Push planner and wa_stream_ref: a 0.5 s recording fed in packets of 1, 7, K/2 - 1, K/2, K, 160 and 4800 frames (at most what a ring of 4096
   samples takes: 1984 frames at 8 kHz, 4032 at 16 kHz) and in a seeded irregular split, at 8, 16, 22.05, 44.1 and 48 kHz, I16 and F32, mono and
   stereo: what the pushes and the flush make final, written to a ring of 4096 samples and gathered back, is wa_audio_ref on the whole
   recording bit for bit, and the output count after every push is ceil((T - K/2) L / M) (0 up to T = K/2; T at 16 kHz), ceil(T L / M) after
   the flush.
5. Deliberately wrong variants each change an expected value: an output released one frame early, a carry one frame short, the commit taken on
   iter % n_new_line == 1, take computed from n_len alone.  The first two move a sample by one tap at the filter's edge, where the Kaiser
   window is near zero: they are caught where that product survives F32 rounding - in some cases, counted and printed, not in every one.
6. The driver built with -fsanitize=address,undefined runs clean as a stand-alone program and prints the same.
7. The code object wa_stream_k.o holds the 5 kernels and none has scratch or a spilled register.
CPU only."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stream_ref import StreamRef  # noqa: E402

SRC = os.path.join(ROOT, "tests", "native", "stream_plan.cpp")
INC = "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc")
BUILD = os.path.join(ROOT, "whisper-rust_amd", "build")
TOOLS = "/opt/rocm/lib/llvm/bin"

TRIPLES = [(1000, 10000, 200), (3000, 10000, 200), (500, 5000, 200), (3000, 3000, 0), (700, 2000, 900), (1000, 1000, 1000), (1000, 4000, 200),
           (2000, 5000, 300)]
N_WINDOWS = 14
RATES = [8000, 16000, 22050, 44100, 48000]
I16, F32 = 0, 1
RING = 4096


def plan_of(rate):
    g = math.gcd(rate, 16000)
    L, M = 16000 // g, rate // g
    return L, M, 0 if rate == 16000 else 64 * -(-max(L, M) // L)


def final_of(rate, T):
    L, M, K = plan_of(rate)
    if K == 0:
        return T
    return 0 if T <= K // 2 else -(-(T - K // 2) * L // M)


def splits_of(rate, n_frames, rng):
    K = plan_of(rate)[2] or 64
    out = {}
    L, M = plan_of(rate)[:2]
    for p in (1, 7, K // 2 - 1, K // 2, K, 160, 4800):
        p = min(p, RING * M // L - K)               # a packet's outputs fit the ring: 1984 frames at 8 kHz, 4032 at 16 kHz
        out["p%d" % p] = [p] * (n_frames // p) + ([n_frames % p] if n_frames % p else [])
    cuts = np.sort(rng.choice(np.arange(1, n_frames), 37, replace=False))
    out["irregular"] = list(np.diff(np.concatenate([[0], cuts, [n_frames]])))
    return out


def make_input(rng, n_frames, ch, fmt):
    n = n_frames * ch
    if fmt == I16:
        return rng.integers(-32768, 32768, n).astype(np.int16)
    return rng.uniform(-1.0, 1.0, n).astype(np.float32)


class Driver:
    def __init__(self, exe, work):
        self.exe, self.work, self.n = exe, work, 0

    def run(self, lines):
        self.n += 1
        cmd = str(self.work / ("cmd_%d.txt" % self.n))
        with open(cmd, "w") as f:
            f.write("".join(l + "\n" for l in lines))
        r = subprocess.run([self.exe, cmd], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
        return r.stdout.splitlines(), cmd


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    work = tmp_path_factory.mktemp("stream_plan")
    exe = str(work / "stream_plan")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", INC, SRC, "-o", exe])
    drv = Driver(exe, work)
    # every push case once: (rate, fmt, ch) -> input, whole-recording reference, per split the outputs of the right rule (0) and the wrong ones (1, 2)
    rng = np.random.default_rng(20241021)
    cases, lines = {}, []
    for r in RATES:
        n_frames = r // 2
        for fmt in (I16, F32):
            for ch in (1, 2):
                key = (r, fmt, ch)
                x = make_input(rng, n_frames, ch, fmt)
                inp = str(work / ("in_%d_%d_%d.bin" % key))
                x.tofile(inp)
                whole = str(work / ("whole_%d_%d_%d.bin" % key))
                lines.append("whole %d %d %d %d %s %s" % (r, fmt, ch, n_frames, inp, whole))
                c = dict(n_frames=n_frames, whole=whole, splits={})
                for name, packets in splits_of(r, n_frames, rng).items():
                    sp = str(work / ("split_%d_%d_%d_%s.bin" % (key + (name,))))
                    np.asarray(packets, np.int64).tofile(sp)
                    runs = {}
                    for var in ([0] if r == 16000 else [0, 1, 2]):
                        o = str(work / ("out_%d_%d_%d_%s_v%d.bin" % (key + (name, var))))
                        cn = str(work / ("cnt_%d_%d_%d_%s_v%d.bin" % (key + (name, var))))
                        lines.append("push %d %d %d %d %s %s %s %s %d" % (r, fmt, ch, n_frames, inp, sp, o, cn, var))
                        runs[var] = (o, cn)
                    c["splits"][name] = dict(packets=packets, runs=runs)
                cases[key] = c
    out, cmd = drv.run(lines)
    at = 0
    for key, c in cases.items():
        tag, n = out[at].split(); at += 1
        assert tag == "whole"
        c["whole"] = np.fromfile(c["whole"], np.float32)
        assert len(c["whole"]) == int(n)
        for name, s in c["splits"].items():
            for var, (o, cn) in s["runs"].items():
                tag, n = out[at].split(); at += 1
                assert tag == "push"
                s["runs"][var] = (np.fromfile(o, np.float32) if int(n) else np.zeros(0, np.float32), np.fromfile(cn, np.int64))
    return dict(work=work, drv=drv, cases=cases, cmd=cmd, stdout=out)


def literal_windows(step, length, keep):
    ref = StreamRef(step, length, keep)
    audio = np.arange(N_WINDOWS * ref.n_samples_step, dtype=np.float32)     # exact in F32 up to 2^24: 14 x 48000 is less
    rows = []
    for k, new in enumerate(ref.steps(audio)):
        pcm = ref.window(new)
        e = (k + 1) * ref.n_samples_step
        assert len(pcm) <= ref.n_samples_keep + ref.n_samples_len
        assert np.array_equal(pcm, np.arange(e - len(pcm), e, dtype=np.float32)), "the literal window is not the range [e - len, e)"
        rows.append((ref.n_samples_take, len(pcm), 1 if ref.after([]) else 0, 1, e - len(pcm)))
    assert len(rows) == N_WINDOWS
    return ref, rows


def driver_windows(drv, step, length, keep, var):
    out, _ = drv.run(["sizes %d %d %d" % (step, length, keep), "plan %d %d %d %d %d" % (step, length, keep, N_WINDOWS, var)])
    return out[0].split(), [tuple(int(v) for v in l.split()[1:]) for l in out[1:]]


@pytest.mark.parametrize("triple", TRIPLES)
def test_plan_is_the_literal_restatement(env, triple):
    ref, want = literal_windows(*triple)
    sizes, got = driver_windows(env["drv"], *triple, 0)
    assert sizes == ["sizes", "ok", str(ref.n_samples_step), str(ref.n_samples_len), str(ref.n_samples_keep), str(ref.n_new_line)]
    assert got == want
    assert any(r[2] for r in want) and (ref.n_new_line == 1 or not all(r[2] for r in want))


def test_refused_sizes(env):
    out, _ = env["drv"].run(["sizes 0 10000 200", "sizes -5 10000 200", "sizes 1000 29801 200", "sizes 1000 29800 200", "sizes 30000 1000 0",
                             "sizes 30001 1000 0", "sizes 20000 1000 20000"])
    a, b = StreamRef(1000, 29800, 200), StreamRef(30000, 1000, 0)
    assert out == ["sizes refused", "sizes refused", "sizes refused", "sizes ok %d %d %d 28" % (a.n_samples_step, a.n_samples_len, a.n_samples_keep),
                   "sizes ok %d %d 0 1" % (b.n_samples_step, b.n_samples_len), "sizes refused", "sizes refused"]


def test_wrong_commit_and_take_change_the_windows(env):
    caught = {3: 0, 4: 0}
    for triple in TRIPLES:
        _, want = literal_windows(*triple)
        for var in (3, 4):
            _, got = driver_windows(env["drv"], *triple, var)
            caught[var] += got != want
    print("triples on which the wrong variant changes a window: commit %d, take %d of %d" % (caught[3], caught[4], len(TRIPLES)))
    assert caught[3] == len(TRIPLES)            # the commit flag itself moves wherever n_new_line > 1, and is never set where it is 1
    assert caught[4] >= 1                       # only where n_keep + n_len - n_step binds: a line is committed before the windows reach it elsewhere


@pytest.mark.parametrize("triple", [(1000, 4000, 200), (3000, 10000, 200), (700, 2000, 900)])
def test_drop_rule(env, triple):
    ref, rows = literal_windows(*triple)
    ns, nk, nl = ref.n_samples_step, ref.n_samples_keep, ref.n_samples_len
    out, _ = env["drv"].run(["drop %d %d %d %d" % (triple + (2 * ns,)), "drop %d %d %d %d" % (triple + (2 * ns + 1,))])
    assert out[0] == "drop 0 1"                                          # nothing dropped, the third window ran
    assert out[1].split()[:5] == ["win"] + [str(v) for v in rows[2][:4]]
    assert out[2] == "drop %d 0" % (2 * ns + 1)
    old = rows[1][1] if not rows[1][2] else min(nk, rows[1][1])           # what the second window left
    take = min(old, max(0, nk + nl - ns))
    e = 2 * ns
    commit = 1 if 3 % ref.n_new_line == 0 else 0                          # the dropped step ran no window: this is the third
    if take > 0:
        assert out[3] == "win %d %d %d 2 %d %d %d %d" % (take, take + ns, commit, e - take, take, e + 2 * ns + 1, ns)
    else:
        assert out[3] == "win 0 %d %d 1 %d %d -1 -1" % (ns, commit, e + 2 * ns + 1, ns)


def test_ring_pieces(env):
    cap = 1000
    out, _ = env["drv"].run(["ring %d %d %d" % t for t in [(900, 100, cap), (2000, 300, cap), (3000, 1000, cap), (2700, 500, cap), (999, 2, cap),
                                                          (5999, 1, cap), (123, 0, cap)]])
    assert out == ["ring 1 900 100 -1 -1", "ring 1 0 300 -1 -1", "ring 1 0 1000 -1 -1", "ring 2 700 300 0 200", "ring 2 999 1 0 1", "ring 1 999 1 -1 -1",
                   "ring 0 -1 -1 -1 -1"]


def test_final_counts(env):
    pairs = [(r, T) for r in RATES for T in (0, 1, (plan_of(r)[2] or 64) // 2, (plan_of(r)[2] or 64) // 2 + 1, 4800, 2 ** 40 + 1)]
    out, _ = env["drv"].run(["final %d %d 0" % p for p in pairs])
    assert out == ["final %d" % final_of(*p) for p in pairs]


def test_packets_give_the_whole_recording(env):
    seen = 0
    for (r, fmt, ch), c in env["cases"].items():
        L, M, K = plan_of(r)
        assert len(c["whole"]) == -(-c["n_frames"] * L // M)
        for name, s in c["splits"].items():
            got, counts = s["runs"][0]
            assert got.tobytes() == c["whole"].tobytes(), (r, fmt, ch, name)
            T = np.cumsum(np.asarray(s["packets"], np.int64))
            want = [final_of(r, int(t)) for t in T] + [len(c["whole"])]
            assert counts.tolist() == want, (r, fmt, ch, name)
            seen += 1
    assert seen == len(RATES) * 4 * 8


def test_wrong_release_and_carry_change_the_outputs(env):
    caught, runs = {1: 0, 2: 0}, 0
    for (r, fmt, ch), c in env["cases"].items():
        if r == 16000:
            continue
        for name, s in c["splits"].items():
            runs += 1
            for var in (1, 2):
                got, counts = s["runs"][var]
                caught[var] += got.tobytes() != c["whole"].tobytes()
                if var == 1 and len(s["packets"]) > 1:          # released early: the counts themselves are ahead
                    assert counts.tolist() != s["runs"][0][1].tolist(), (r, fmt, ch, name)
    print("push runs in which the wrong variant changes a sample: early release %d, short carry %d of %d" % (caught[1], caught[2], runs))
    assert caught[1] > 0 and caught[2] > 0


def test_sanitized_driver_runs_clean(env):
    exe = str(env["work"] / "stream_plan_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", INC, SRC, "-o", exe])
    r = subprocess.run([exe, env["cmd"]], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.splitlines() == env["stdout"]
    lines = ["plan %d %d %d %d 0" % (t + (N_WINDOWS,)) for t in TRIPLES] + ["drop 1000 4000 200 32001", "ring 2700 500 1000"]
    cmd = str(env["work"] / "cmd_san.txt")
    open(cmd, "w").write("".join(l + "\n" for l in lines))
    r = subprocess.run([exe, cmd], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.splitlines() == env["drv"].run(lines)[0]


def test_stream_kernels_use_no_scratch(tmp_path):
    """Read from the code object the build just made, as tests/test_audio_math.py reads wa_audio_k.o."""
    if not os.path.exists(os.path.join(BUILD, "wa_quantk.o")):
        pytest.skip("no build tree here")
    obj = os.path.join(BUILD, "wa_stream_k.o")
    assert os.path.exists(obj), "the build made wa_quantk.o but not wa_stream_k.o"
    fat, co = str(tmp_path / "fat"), str(tmp_path / "co")
    subprocess.check_call([os.path.join(TOOLS, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, obj])
    subprocess.check_call([os.path.join(TOOLS, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co])
    notes = subprocess.check_output([os.path.join(TOOLS, "llvm-readelf"), "--notes", co], text=True)
    seen, name = {}, None
    for line in notes.splitlines():
        line = line.strip()
        if line.startswith(".name:"):
            name = line.split(":", 1)[1].strip()
        elif name and (line.startswith(".private_segment_fixed_size:") or line.startswith(".vgpr_spill_count:") or line.startswith(".sgpr_spill_count:")):
            seen.setdefault(name, {})[line.split(":")[0]] = int(line.split(":")[1])
    assert len([k for k in seen if "k_stream_push" in k]) == 4 and len([k for k in seen if "k_stream_window" in k]) == 1 and len(seen) == 5, sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

"""The audio front end's host code (whisper-rust_amd/csrc/wa_audio.h through tests/native/audio_math.cpp, g++ alone: no HIP, no device).

1. The filter of every supported rate, in float64 on the F32 taps as the library builds them: the gain at and beyond the lower rate's Nyquist
   frequency is below 1 / 32768 (-90.3 dB: a full-scale tone there leaves less than one 16-bit step), every phase sums to 1 within K 2^-24.
2. wa_audio_ref against a float64 polyphase evaluation with the same taps: per sample |y32 - y64| <= (K + 2) 2^-24 sum_k |h_k| |x_k| (K fmaf
   roundings of partial sums that never exceed sum |h||x|, first order, with two more for slack of the higher-order terms; the float64 sum's own error is
   2^-29 of that); output lengths at n_frames 0, 1, K/2 - 1, K and a prime near 10 000.
3. At 16 kHz the output is bit-identical to the numpy restatements of whisper-rs' utilities.rs formulas, +-32767 and -32768 included.
4. Deliberately wrong loops in the driver (phase off by one, taps reversed, i0 rounded up) change the expected values of every resampling case
   they apply to: the comparison of 2. and of tests/test_audio_kernels_gpu.py is not vacuous.
5. The driver built with -fsanitize=address,undefined runs clean as a stand-alone program and prints the same.
6. The code object wa_audio_k.o holds the 8 kernels and none has scratch or a spilled register.
CPU only."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper-rust_amd"))
import whisper_rs as W  # noqa: E402  (the numpy restatements only: no library is loaded here)

SRC = os.path.join(ROOT, "tests", "native", "audio_math.cpp")
INC = "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc")
BUILD = os.path.join(ROOT, "whisper-rust_amd", "build")
TOOLS = "/opt/rocm/lib/llvm/bin"

RATES = [8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000]       # 16000 has no filter
REFUSED_RATES = [0, -16000, 7999, 192001, 16001, 44101, 8001, 11001]                              # out of range, or L > 640
I16, F32 = 0, 1
PRIME = 10007


def plan_of(rate):
    g = math.gcd(rate, 16000)
    L, M = 16000 // g, rate // g
    return L, M, 0 if rate == 16000 else 64 * -(-max(L, M) // L)


def lengths_of(rate):
    K = plan_of(rate)[2] or 64                      # 16 kHz has no taps: the lengths of K = 64
    return [0, 1, K // 2 - 1, K, PRIME]


def make_input(rng, n_frames, ch, fmt):
    n = n_frames * ch
    if fmt == I16:
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[:min(n, 6)] = np.array([32767, -32768, -32767, 32767, -32768, -32768], np.int16)[:min(n, 6)]
        return x
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    x[:min(n, 4)] = np.array([1.0, 1.0, -1.0, -1.0], np.float32)[:min(n, 4)]
    return x


def mono_of(x, ch, fmt):
    if fmt == I16:
        return W.convert_integer_to_float_audio(x) if ch == 1 else W.convert_stereo_i16_to_mono_f32(x)
    return np.asarray(x, np.float32) if ch == 1 else W.convert_stereo_to_mono_audio(x)


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
    work = tmp_path_factory.mktemp("audio_math")
    exe = str(work / "audio_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", INC, SRC, "-o", exe])
    drv = Driver(exe, work)
    # the taps of every rate
    out, _ = drv.run(["taps %d %s" % (r, work / ("taps_%d.bin" % r)) for r in RATES])
    taps = {}
    for r, line in zip(RATES, out):
        tag, L, M, K = line.split()
        assert tag == "taps" and (int(L), int(M), int(K)) == plan_of(r), (r, line)
        taps[r] = np.fromfile(str(work / ("taps_%d.bin" % r)), np.float32).reshape(int(L), int(K))
    # every resampling case once: (rate, fmt, ch, n_frames) -> input, the driver's outputs for the right loops (0, 1) and the wrong ones (2, 3, 4)
    rng = np.random.default_rng(20240607)
    cases, lines = {}, []
    for r in RATES + [16000]:
        for fmt in (I16, F32):
            for ch in (1, 2):
                full = r in (8000, 11025, 16000, 44100, 48000) or (fmt, ch) == (I16, 2)      # every length at these, the prime elsewhere
                for n in (lengths_of(r) if full else [PRIME]):
                    x = make_input(rng, n, ch, fmt)
                    key = (r, fmt, ch, n)
                    inp = str(work / ("in_%d_%d_%d_%d.bin" % key))
                    x.tofile(inp)
                    cases[key] = dict(x=x, out={})
                    for var in ([0] if r == 16000 else [0, 1, 2, 3, 4]):
                        o = str(work / ("out_%d_%d_%d_%d_v%d.bin" % (key + (var,))))
                        lines.append("ref %d %d %d %d %s %s %d" % (r, fmt, ch, n, inp, o, var))
                        cases[key]["out"][var] = o
    out, cmd = drv.run(lines)
    at = 0
    for key, c in cases.items():
        for var, o in c["out"].items():
            tag, n = out[at].split(); at += 1
            assert tag == "ref"
            c["out"][var] = np.fromfile(o, np.float32) if int(n) > 0 else np.zeros(0, np.float32)
            assert len(c["out"][var]) == int(n)
    return dict(work=work, drv=drv, taps=taps, cases=cases, cmd=cmd, stdout=out)


def response(t, L, M, K):
    """|H(f)| / L of the prototype on the grid of rate 16000 M, f in cycles per sample of that grid; float64 on the F32 taps"""
    proto = np.zeros(K * L)
    k = np.arange(K)
    for p in range(L):
        proto[(K - 1 - k) * L + p] = t[p].astype(np.float64)          # instant (K/2 - 1 - k) L + p, moved up by (K/2) L
    nfft = 1 << int(np.ceil(np.log2(len(proto) * 16)))
    return np.abs(np.fft.rfft(proto, nfft)) / L, np.arange(nfft // 2 + 1) / nfft


@pytest.mark.parametrize("rate", RATES)
def test_stop_band_and_phase_sums(env, rate):
    L, M, K = plan_of(rate)
    t = env["taps"][rate]
    H, f = response(t, L, M, K)
    nyq = 0.5 / max(L, M)                                   # the lower rate's Nyquist frequency on that grid
    stop = H[f >= nyq * (1 - 1e-12)].max()
    edge = f[np.argmax(H < 10 ** (-0.1 / 20))] * 16000 * M
    sums = t.astype(np.float64).sum(axis=1)
    print("rate %6d  L %3d M %3d K %3d  table %3d KB  stop band %.2f dB  -0.1 dB edge %.0f Hz  phase sums within %.2e (bound %.2e)"
          % (rate, L, M, K, L * K * 4 // 1024, 20 * np.log10(stop), edge, np.abs(sums - 1).max(), K * 2.0 ** -24))
    assert stop < 1.0 / 32768.0, 20 * np.log10(stop)
    assert np.abs(sums - 1).max() <= K * 2.0 ** -24
    assert L * K * 4 <= 160 * 1024


def test_plans_and_refused_rates(env):
    out, _ = env["drv"].run(["plan %d" % r for r in RATES + [16000] + REFUSED_RATES])
    for r, line in zip(RATES + [16000], out):
        L, M, K = plan_of(r)
        got = line.split()
        assert got[:5] == ["plan", "ok", str(L), str(M), str(K)], (r, line)
        assert int(got[5]) <= 14336, "the span of a tile does not fit the kernel's LDS"
    assert out[len(RATES) + 1:] == ["plan refused"] * len(REFUSED_RATES)


def test_output_lengths(env):
    pairs = [(n, r) for r in RATES + [16000] for n in lengths_of(r) + [2 ** 40 + 1]]
    out, _ = env["drv"].run(["nout %d %d" % p for p in pairs] + ["nout -1 48000", "nout 5 16001", "nout %d 48000" % (2 ** 62)])
    for (n, r), line in zip(pairs, out):
        assert line == "nout %d" % (-(-n * 16000 // r)), (n, r, line)
    assert out[len(pairs):] == ["nout -1"] * 3
    for (r, fmt, ch, n), c in env["cases"].items():
        assert len(c["out"][0]) == -(-n * 16000 // r)


def float64_polyphase(x_mono, t, L, M, K, n_out):
    """y64[n] and the bound's sum_k |h_k| |x_k|, with the taps and the samples as exact float64 values"""
    n = np.arange(n_out, dtype=np.int64)
    tt = n * M
    p, i0 = tt % L, tt // L
    idx = (i0 - K // 2 + 1)[:, None] + np.arange(K)[None, :]
    xp = np.concatenate([np.zeros(K), x_mono.astype(np.float64), np.zeros(K)])
    xs = xp[idx + K]
    h = t.astype(np.float64)[p]
    return (h * xs).sum(axis=1), (np.abs(h) * np.abs(xs)).sum(axis=1)


def test_restatement_against_float64(env):
    worst = 0.0
    for (r, fmt, ch, n), c in env["cases"].items():
        if r == 16000 or n == 0:
            continue
        L, M, K = plan_of(r)
        y32 = c["out"][0]
        y64, mag = float64_polyphase(mono_of(c["x"], ch, fmt), env["taps"][r], L, M, K, len(y32))
        bound = (K + 2) * 2.0 ** -24 * mag
        err = np.abs(y32.astype(np.float64) - y64)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (r, fmt, ch, n, float((err - bound).max()))
        assert np.all(np.isfinite(y32))
    print("largest |y32 - y64| / bound over all cases: %.3f" % worst)
    assert worst > 0.0                                       # the comparison saw rounding at all


def test_conversion_is_the_utilities_formulas(env):
    seen = 0
    for (r, fmt, ch, n), c in env["cases"].items():
        if r != 16000:
            continue
        want = mono_of(c["x"], ch, fmt)
        assert c["out"][0].tobytes() == want.tobytes(), (fmt, ch, n)
        seen += 1
    assert seen == 4 * len(lengths_of(16000))
    # the extreme values, alone and paired
    ext = np.array([32767, -32768, -32767, 32767, -32768, -32768, 32767, 32767, 0, 1, -1, 0], np.int16)
    assert W.convert_integer_to_float_audio(ext)[1] == -1.0 and W.convert_stereo_i16_to_mono_f32(ext)[2] == -1.0
    assert W.convert_stereo_i16_to_mono_f32(ext)[3] == np.float32(32767.0 / 32768.0)


def test_wrong_loops_change_every_resampling_case(env):
    caught = {2: 0, 3: 0, 4: 0}
    for (r, fmt, ch, n), c in env["cases"].items():
        if r == 16000 or n == 0:
            continue
        L = plan_of(r)[0]
        right = c["out"][0].tobytes()
        assert c["out"][1].tobytes() == right, "the driver's own loop differs from wa_audio_ref: %r" % ((r, fmt, ch, n),)
        for var in (2, 3, 4):
            if (var != 3 and L == 1) or (var == 4 and len(c["out"][0]) == 1):
                assert c["out"][var].tobytes() == right             # one phase, or t / L exact (as at n = 0): here they are the right loop
                continue
            assert c["out"][var].tobytes() != right, (var, r, fmt, ch, n)
            caught[var] += 1
    assert min(caught.values()) > 20, caught


def test_sanitized_driver_runs_clean(env):
    exe = str(env["work"] / "audio_math_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", INC, SRC, "-o", exe])
    r = subprocess.run([exe, env["cmd"]], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-3000:]
    assert r.stdout.splitlines() == env["stdout"]
    for (key, c) in env["cases"].items():                       # the sanitised run rewrote the outputs: they are the same
        o = str(env["work"] / ("out_%d_%d_%d_%d_v0.bin" % key))
        got = np.fromfile(o, np.float32) if len(c["out"][0]) else np.zeros(0, np.float32)
        assert got.tobytes() == c["out"][0].tobytes(), key


def test_audio_kernels_use_no_scratch(tmp_path):
    """Read from the code object the build just made, as tests/test_kquant_fewrows_math.py reads wa_quantk_rows.o."""
    if not os.path.exists(os.path.join(BUILD, "wa_quantk.o")):
        pytest.skip("no build tree here")
    obj = os.path.join(BUILD, "wa_audio_k.o")
    assert os.path.exists(obj), "the build made wa_quantk.o but not wa_audio_k.o"
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
    assert len([k for k in seen if "k_audio_convert" in k]) == 4 and len([k for k in seen if "k_audio_resample" in k]) == 4 and len(seen) == 8, sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

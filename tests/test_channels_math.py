"""The host code of the two-channel calls (whisper-rust_amd/csrc/wa_channels.h through tests/native/channels_math.cpp, g++ alone: no HIP, no device).

1. wa_ch_split_ref: plane c equals, bit for bit, wa_audio_ref on channel c extracted and presented as a MONO recording; int16 and F32 at
   16 000, 8 000 (L 2, M 1), 44 100 (L 160, M 441) and 48 000 (L 1, M 3) Hz.
2. wa_ch_energy_ref, the fixed summation order, against two yardsticks that know nothing of that order: samples that are multiples of
   2^-10 in [-1, 1], where every order gives the exact sum, against integer arithmetic (equality); random N(0, 0.1) samples against numpy's
   sequential float64 cumsum of |x|, relative difference <= n 2^-53 (two sums of the same n non-negative terms, each with at most n - 1
   roundings of 2^-53 relative on any path and no cancellation: first order).
3. The label rule on built energy ratios 2, 1/2, 1, 1.05, 1/1.05 and both-zero; every case is first shown to lie at least 1e-6 relative
   from both thresholds, so that no summation order could decide it.
4. The cli's centisecond rule at t = 0, beyond the end and negative; the gate; the merge order and the clamps on hand-written lists, one
   of them with a clamp that pushes a t0 past its own t1.
5. Two planes of the widest span fit the split kernel's LDS at every supported rate; the code object holds the five kernels without scratch.
CPU only."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "channels_math.cpp")
INC = "-I" + os.path.join(ROOT, "whisper-rust_amd", "csrc")
BUILD = os.path.join(ROOT, "whisper-rust_amd", "build")
TOOLS = "/opt/rocm/lib/llvm/bin"

RATES = [16000, 8000, 44100, 48000]
ALL_RATES = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000]
I16, F32 = 0, 1
LENGTHS = [0, 1, 2, 7, 97, 4099]


def make_stereo(rng, n_frames, fmt):
    """interleaved stereo, the two channels independent draws"""
    if fmt == I16:
        x = rng.integers(-32768, 32768, 2 * n_frames).astype(np.int16)
        x[:min(len(x), 4)] = np.array([32767, -32768, -32768, 32767], np.int16)[:min(len(x), 4)]
        return x
    return rng.uniform(-1.0, 1.0, 2 * n_frames).astype(np.float32)


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
        return r.stdout.splitlines()

    def energy(self, x, spans):
        self.n += 1
        ip, op = str(self.work / ("plane_%d.bin" % self.n)), str(self.work / ("energy_%d.bin" % self.n))
        np.asarray(x, np.float32).tofile(ip)
        out = self.run(["energy %s %s %s" % (ip, op, " ".join("%d %d" % s for s in spans))])
        assert out == ["energy %d" % len(spans)]
        return np.fromfile(op, np.float64) if spans else np.zeros(0)


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    assert shutil.which("g++"), "g++ is missing: the build itself needs it"
    work = tmp_path_factory.mktemp("channels_math")
    exe = str(work / "channels_math")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", INC, SRC, "-o", exe])
    return Driver(exe, work)


@pytest.fixture(scope="module")
def consts(drv):
    tag, tile, lds, lanes, align = drv.run(["const"])[0].split()
    assert tag == "const"
    return dict(tile=int(tile), lds=int(lds), lanes=int(lanes), align=int(align))


# ---- 1. the split ----
@pytest.mark.parametrize("rate", RATES)
def test_split_is_the_mono_front_end_per_channel(drv, consts, rate):
    rng = np.random.default_rng(31 + rate)
    lines, cases = [], []
    for fmt in (I16, F32):
        for n in LENGTHS:
            x = make_stereo(rng, n, fmt)
            ip = str(drv.work / ("st_%d_%d_%d.bin" % (rate, fmt, n)))
            x.tofile(ip)
            outs = [str(drv.work / ("st_%d_%d_%d_%s.bin" % (rate, fmt, n, k))) for k in ("p0", "p1", "m0", "m1")]
            lines += ["split %d %d %d %s %s %s" % (rate, fmt, n, ip, outs[0], outs[1]),
                      "mono %d %d %d %s 0 %s" % (rate, fmt, n, ip, outs[2]), "mono %d %d %d %s 1 %s" % (rate, fmt, n, ip, outs[3])]
            cases.append((fmt, n, x, outs))
    out = drv.run(lines)
    for k, (fmt, n, x, outs) in enumerate(cases):
        n_out = -(-n * 16000 // rate)
        stride = -(-n_out // consts["align"]) * consts["align"]
        assert out[3 * k:3 * k + 3] == ["split %d %d" % (n_out, stride), "mono %d" % n_out, "mono %d" % n_out], (rate, fmt, n)
        if n_out == 0:
            continue
        p0, p1, m0, m1 = (np.fromfile(o, np.uint32) for o in outs)
        assert len(p0) == len(p1) == n_out
        assert np.array_equal(p0, m0) and np.array_equal(p1, m1), (rate, fmt, n)
        assert not np.array_equal(p0, p1)                       # the channels are different signals: a swap or a mix would show above
        if rate == 16000:                                       # and at 16 kHz a plane is the channel itself
            ch = x.reshape(-1, 2).T
            want = [(c.astype(np.float32) / np.float32(32768.0)) if fmt == I16 else c for c in ch]
            assert np.array_equal(p0, want[0].view(np.uint32)) and np.array_equal(p1, want[1].view(np.uint32))


def test_a_silent_channel_is_plus_zero(drv):
    """channel 1 all zero: plane 1 is +0.0 everywhere (a negative tap times zero is -0.0, and -0.0 + 0.0 = +0.0), plane 0 is not disturbed"""
    rng = np.random.default_rng(5)
    for rate in RATES:
        for fmt in (I16, F32):
            x = make_stereo(rng, 1500, fmt)
            x[1::2] = 0
            ip, o0, o1 = (str(drv.work / ("z_%d_%d_%s.bin" % (rate, fmt, k))) for k in ("in", "p0", "p1"))
            x.tofile(ip)
            drv.run(["split %d %d 1500 %s %s %s" % (rate, fmt, ip, o0, o1)])
            assert not np.fromfile(o1, np.uint32).any(), (rate, fmt)
            assert np.fromfile(o0, np.uint32).any()


# ---- 2. the energy order ----
def spans_for(n, lanes):
    return [(0, 0), (5, 5), (9, 3), (0, 1), (n - 1, n), (0, n), (3, lanes), (3, lanes - 1), (3, lanes + 1), (lanes, 2 * lanes), (lanes - 1, 3 * lanes + 7),
            (-50, 40), (n - 40, n + 1000), (n, n + 5), (1234, 98765 if n > 98765 else n - 3)]


def test_energy_exact_on_dyadic_samples(drv, consts):
    """multiples of 2^-10 in [-1, 1]: every partial sum is a multiple of 2^-10 below 2^53 2^-10, so every order gives the exact sum"""
    rng = np.random.default_rng(77)
    n = 480000
    k = rng.integers(-1024, 1025, n)
    k[:4] = [1024, -1024, 0, 1]
    x = (k / 1024.0).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 1024.0, k)
    spans = spans_for(n, consts["lanes"])
    got = drv.energy(x, spans)
    for (a, b), e in zip(spans, got):
        a, b = max(a, 0), min(b, n)
        want = int(np.abs(k[a:b]).sum()) if a < b else 0
        assert e * 1024.0 == want, (a, b, e, want)
        assert a < b or (e == 0.0 and not np.signbit(e))


def test_energy_against_a_sequential_sum(drv, consts):
    rng = np.random.default_rng(78)
    n = 480000
    x = rng.normal(0.0, 0.1, n).astype(np.float32)
    spans = [s for s in spans_for(n, consts["lanes"]) if max(s[0], 0) < min(s[1], n)]
    got = drv.energy(x, spans)
    worst = 0.0
    for (a, b), e in zip(spans, got):
        a, b = max(a, 0), min(b, n)
        seq = np.cumsum(np.abs(x[a:b]).astype(np.float64))[-1]
        rel = abs(e - seq) / seq
        worst = max(worst, rel / ((b - a) * 2.0 ** -53))
        assert rel <= (b - a) * 2.0 ** -53, (a, b, e, seq)
        if b - a == 1:
            assert e == float(abs(x[a]))
    print("largest |fixed order - sequential| / (n 2^-53 sequential) = %.3g" % worst)


# ---- 3. labels ----
LABEL_CASES = [(2.0, 0), (0.5, 1), (1.0, -1), (1.05, -1), (1.0 / 1.05, -1)]


def test_labels_on_built_ratios(drv):
    """plane 1 is 0.25 everywhere, plane 0 is ratio x 0.25: the energies come from the energy function itself, the thresholds are e0 = 1.1 e1
    and e1 = 1.1 e0; every case is at least 1e-6 relative away from both, far more than the n 2^-53 a summation order can move a sum"""
    n = 1000
    e1 = drv.energy(np.full(n, 0.25, np.float32), [(0, n)])[0]
    lines, want = [], []
    for ratio, label in LABEL_CASES:
        e0 = drv.energy(np.full(n, np.float32(0.25 * ratio), np.float32), [(0, n)])[0]
        assert abs(e0 / e1 - ratio) < 1e-6
        for thr in (1.1 * e1, e1 / 1.1):
            assert abs(e0 - thr) / thr >= 1e-6, (ratio, e0, e1)
        assert n * 2.0 ** -53 < 1e-9
        lines.append("label %s %s 0" % (float(e0).hex(), float(e1).hex()))            # ratio <= 0: the cli's 1.1
        lines.append("label %s %s 1.1" % (float(e0).hex(), float(e1).hex()))
        want += ["label %d" % label] * 2
    z = drv.energy(np.zeros(n, np.float32), [(0, n)])[0]
    assert z == 0.0                                             # a sum of zeros is zero in every order: 0 > 1.1 x 0 is false both ways
    lines += ["label %s %s 0" % (float(z).hex(), float(z).hex()), "label 0x1p+0 0x1p-1 1.5", "label 0x1p+0 0x1p-1 3", "label 0x1p-1 0x1p+0 -2"]
    want += ["label -1", "label 0", "label -1", "label 1"]
    assert drv.run(lines) == want


# ---- 4. the cli's time rule, the gate, the merge ----
def test_centiseconds_to_samples(drv):
    n = 100000
    cases = [(0, 0), (-5, 0), (-2 ** 40, 0), (1, 160), (3, 480), (150, 24000), (624, 99840), (625, n - 1), (626, n - 1), (10 ** 7, n - 1), (2 ** 50, n - 1)]
    assert drv.run(["cs %d %d" % (t, n) for t, _ in cases]) == ["cs %d" % s for _, s in cases]
    assert drv.run(["cs 0 1", "cs 7 1", "cs 10 1601", "cs 10 1600"]) == ["cs 0", "cs 0", "cs 1600", "cs 1599"]


def test_gate(drv):
    cases = [(1.0, 4.0, 0.5, 1), (3.0, 4.0, 0.5, 0), (2.0, 4.0, 0.5, 0), (1.0, 4.0, 0.0, 0), (0.0, 0.0, 0.5, 0), (0.0, 1e-9, 0.5, 1), (5.0, 1.0, 0.5, 0)]
    assert drv.run(["gate %s %s %s" % (float(a).hex(), float(b).hex(), float(g).hex()) for a, b, g, _ in cases]) == ["gate %d" % d for *_, d in cases]


def merge(drv, ch0, ch1):
    line = "merge %d %s %d %s" % (len(ch0), " ".join("%d %d" % s for s in ch0), len(ch1), " ".join("%d %d" % s for s in ch1))
    out = drv.run([line])[0].split()
    assert out[0] == "merge"
    v = [int(t) for t in out[1:]]
    return [tuple(v[i:i + 4]) for i in range(0, len(v), 4)]


def test_merge_order_and_clamps(drv):
    # equal t0 on both channels: channel 0 first; overlapping segments across channels stay as they are
    ch0 = [(100, 300), (300, 450), (900, 905)]
    ch1 = [(100, 250), (200, 400), (420, 900), (900, 1000)]
    got = merge(drv, ch0, ch1)
    assert got == [(0, 0, 100, 300), (1, 0, 100, 250), (1, 1, 250, 400), (0, 1, 300, 450), (1, 2, 420, 900), (0, 2, 900, 910), (1, 3, 900, 1000)]
    # the t0 clamp looked at the previous segment of the SAME channel only: (1, 1) starts at channel 1's 250, not at channel 0's 300;
    # (1, 2) starts at 420 although channel 0's (0, 1) runs until 450
    assert [t0 for *_, t0, _ in got] == sorted(t0 for *_, t0, _ in got)
    # a short segment is stretched to 10 cs before the next one of its channel is clamped against it
    assert merge(drv, [(50, 52), (55, 80)], []) == [(0, 0, 50, 60), (0, 1, 60, 80)]
    # a clamp can reorder nothing inside a channel, but moves a segment behind one of the other channel
    assert merge(drv, [(0, 500), (100, 600)], [(300, 350)]) == [(0, 0, 0, 500), (1, 0, 300, 350), (0, 1, 500, 600)]
    assert merge(drv, [], []) == [] and merge(drv, [], [(5, 30)]) == [(1, 0, 5, 30)]
    # a clamp can push a t0 past its own t1 (t1 is not extended again, as whisper_amd_full_long does not): the next segment of the channel is
    # clamped against that smaller t1 and starts EARLIER - the channel keeps its own order all the same, as whisper_amd_full_long's list does,
    # and the other channel's segments are merged against the heads
    assert merge(drv, [(0, 500), (100, 120), (130, 600)], []) == [(0, 0, 0, 500), (0, 1, 500, 120), (0, 2, 130, 600)]
    assert merge(drv, [(0, 500), (100, 120), (130, 600)], [(50, 90), (200, 300), (550, 560)]) == [
        (0, 0, 0, 500), (1, 0, 50, 90), (1, 1, 200, 300), (0, 1, 500, 120), (0, 2, 130, 600), (1, 2, 550, 560)]


# ---- 5. the kernel's budget ----
def test_two_planes_fit_the_lds_at_every_rate(drv, consts):
    out = drv.run(["span %d" % r for r in ALL_RATES])
    in_lds = []
    for r, line in zip(ALL_RATES, out):
        tag, span, L, K = line.split()
        span4 = (int(span) + 3) & ~3
        assert tag == "span" and 2 * span4 <= consts["lds"], (r, line)
        if int(K) and 2 * span4 + int(L) * int(K) <= consts["lds"]:
            in_lds.append(r)
    assert consts["lds"] * 4 <= 64 * 1024 and consts["tile"] % 256 == 0
    print("taps beside the planes in LDS at", in_lds)
    assert in_lds == [8000, 12000, 24000, 32000, 48000, 96000, 192000]         # the others (L >= 40) keep their 120 .. 160 KB tables in global memory


def test_channel_kernels_use_no_scratch(tmp_path):
    """Read from the code object the build just made, as tests/test_audio_math.py reads wa_audio_k.o."""
    obj = os.path.join(BUILD, "wa_channels_k.o")
    assert os.path.exists(obj), "whisper-rust_amd/build/wa_channels_k.o is missing: __graft_entry__.build() makes it"
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
    assert len([k for k in seen if "k_audio_split" in k]) == 2 and len([k for k in seen if "k_audio_deinterleave" in k]) == 2
    assert len([k for k in seen if "k_channel_energy" in k]) == 1 and len(seen) == 5, sorted(seen)
    for k, v in seen.items():
        assert v == {".private_segment_fixed_size": 0, ".vgpr_spill_count": 0, ".sgpr_spill_count": 0}, (k, v)

"""The streaming sessions' kernels (whisper-rust_amd/csrc/wa_stream.hip) against wa_stream_ref, the host restatement of wa_stream.h, bit for bit.

Through tests/native/libstream_kernels.so: the launchers of the product's own wa_stream_k.o.  tests/test_stream_plan_math.py holds the
restatement to wa_audio_ref on the whole recording and shows that an early release, a short carry, a wrong commit and a wrong take change
the expected values.

k_stream_push: 1.5 s recordings at 8, 16, 22.05, 44.1 and 48 kHz, I16 and F32, mono and stereo, pushed into a ring of 4096 samples (it wraps
five times) in packets of K/2 - 1, K/2, K, 160 and 4800 frames (at most what the ring takes), in a seeded irregular split, in 1- and 7-frame
packets over the first max(3 K, 2 M) frames (every phase of the filter, the packets that release nothing, the first outputs) and in packets that
give tile - 1, tile and tile + 1 new outputs; then the flush.  Every packet is read where it lies in the device copy of the recording, so
its address has whatever alignment the split gives.  The ring is compared whenever it is about to be overwritten and at the end, the carry
with it; the NaN guards around the ring and around both carry buffers must be NaN still.  Full-scale square waves and impulses as well.

k_stream_window: 1, 3 and 8 sessions per launch; windows of 1, tile - 1, tile, tile + 1 and 51 200 samples that do not wrap, wrap, start at
slot 0, end on the last slot, or are two ranges (four pieces where both wrap); sources and destinations 0, 4, 8 and 12 bytes behind a 16-byte
boundary; everything around a destination must be NaN still."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HARNESS = os.path.join(ROOT, "tests", "native", "libstream_kernels.so")
RATES = [8000, 16000, 22050, 44100, 48000]
I16, F32 = 0, 1
COMBOS = [(I16, 1), (I16, 2), (F32, 1), (F32, 2)]
RING = 4096
G = 64
MAX_IMAGES = 16


def plan_of(rate):
    g = math.gcd(rate, 16000)
    L, M = 16000 // g, rate // g
    return L, M, 0 if rate == 16000 else 64 * -(-max(L, M) // L)


def final_of(rate, T):
    L, M, K = plan_of(rate)
    if K == 0:
        return T
    return 0 if T <= K // 2 else -(-(T - K // 2) * L // M)


def cut(n_frames, head, p):
    """`head`, then packets of p frames to the end"""
    rest = n_frames - sum(head)
    return head + [p] * (rest // p) + ([rest % p] if rest % p else [])


def splits_of(rate, n_frames, tile, rng):
    L, M, K = plan_of(rate)
    K = K or 64
    big = RING * M // L - K                         # a packet's outputs fit the ring: 1984 frames at 8 kHz, 4032 at 16 kHz
    out = {}
    for p in (K // 2 - 1, K // 2, K, 160, 4800):
        out["p%d" % p] = cut(n_frames, [], min(p, big))
    small = max(3 * K, 2 * M)
    out["p1"] = cut(n_frames, [1] * small, big)
    out["p7"] = cut(n_frames, [7] * (small // 7), big)
    cuts = np.sort(rng.choice(np.arange(1, n_frames), 61, replace=False))
    out["irregular"] = []
    for v in np.diff(np.concatenate([[0], cuts, [n_frames]])):
        out["irregular"] += cut(int(v), [], big)    # a gap larger than the ring takes is cut
    head, T = [K], K                                # tile - 1, tile, tile + 1 new outputs, where the rate has such a packet
    for want in (tile - 1, tile, tile + 1):
        F = next((F for F in range(1, 4 * tile * M // L + 8) if final_of(rate, T + F) - final_of(rate, T) == want), None)
        if F is not None:
            head.append(F); T += F
    assert len(head) >= 2                           # 8 kHz gives even counts only: the tile itself
    out["tile"] = cut(n_frames, head, 160)
    for name, s in out.items():
        assert sum(s) == n_frames and min(s) > 0, name
    return out


def random_input(rng, n_frames, ch, fmt):
    n = n_frames * ch
    if fmt == I16:
        x = rng.integers(-32768, 32768, n).astype(np.int16)
        x[:6] = np.array([32767, -32768, -32767, 32767, -32768, -32768], np.int16)
        return x
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    x[:4] = np.array([1.0, 1.0, -1.0, -1.0], np.float32)
    return x


def square_input(n_frames, ch, fmt, period=37):
    s = np.where((np.arange(n_frames) // period) % 2 == 0, 1, -1)
    x = np.repeat(s, ch)
    return np.where(x > 0, 32767, -32768).astype(np.int16) if fmt == I16 else x.astype(np.float32)


def impulse_input(n_frames, ch, fmt, spacing):
    at = np.arange(spacing // 2, n_frames, spacing)
    s = np.zeros(n_frames, np.int64)
    s[at] = np.where(np.arange(len(at)) % 2 == 0, 1, -1)
    x = np.repeat(s, ch)
    return np.where(x > 0, 32767, np.where(x < 0, -32768, 0)).astype(np.int16) if fmt == I16 else x.astype(np.float32)


class Harness:
    def __init__(self):
        lib = self.lib = C.CDLL(HARNESS)
        lib.stest_tile.restype = C.c_int
        lib.stest_final.restype = C.c_longlong
        lib.stest_final.argtypes = [C.c_int, C.c_longlong]
        lib.stest_carry_len.restype = C.c_int
        lib.stest_carry_len.argtypes = [C.c_int]
        lib.stest_image_len.restype = C.c_longlong
        lib.stest_image_len.argtypes = [C.c_int, C.c_longlong]
        lib.stest_push_run.restype = C.c_longlong
        lib.stest_push_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_int]
        lib.stest_window_run.restype = C.c_int
        lib.stest_window_run.argtypes = [C.c_int, C.c_void_p, C.c_longlong] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_longlong]

    def push(self, rate, fmt, ch, x, n_frames, packets, where):
        img = self.lib.stest_image_len(rate, RING)
        out = np.zeros((MAX_IMAGES, img), np.float32)
        pk = np.asarray(packets, np.int64)
        n = self.lib.stest_push_run(rate, fmt, ch, x.ctypes.data, n_frames, pk.ctypes.data, len(pk), RING, where, out.ctypes.data, MAX_IMAGES)
        assert n > 0, "stest_push_run returned %d (-1 refused, -2 HIP error, -3 launcher refused, -5 too many images)" % n
        return out[:n]

    def window(self, ring, specs, where):
        """specs: [(pieces [(slot, len)], src_off, dst_off)]; returns the rows [n][row]"""
        n = len(specs)
        longest = max(sum(l for _, l in p) for p, _, _ in specs)
        row = (2 * G + 3 + longest + 3) // 4 * 4
        npc = np.array([len(p) for p, _, _ in specs], np.int32)
        slot, plen = np.zeros((n, 4), np.int32), np.zeros((n, 4), np.int32)
        for i, (p, _, _) in enumerate(specs):
            for q, (s, l) in enumerate(p):
                slot[i, q], plen[i, q] = s, l
        so = np.array([s for _, s, _ in specs], np.int32)
        do = np.array([d for _, _, d in specs], np.int32)
        out = np.zeros((n, row), np.float32)
        r = self.lib.stest_window_run(n, ring.ctypes.data, len(ring), npc.ctypes.data, slot.ctypes.data, plen.ctypes.data, so.ctypes.data, do.ctypes.data,
                                      where, out.ctypes.data, row)
        assert r == 0, "stest_window_run returned %d (-1 refused, -2 HIP error, -3 launcher refused)" % r
        return out


@pytest.fixture(scope="module")
def har():
    assert os.path.exists(HARNESS), "tests/native/libstream_kernels.so is not built (whisper-rust_amd/Makefile: stream_harness)"
    return Harness()


@pytest.fixture(scope="module")
def tile(amd_lib, har):
    t = amd_lib.whisper_amd_stream_tile()
    assert t == har.lib.stest_tile() and t >= 256 and t % 256 == 0
    return t


def check_images(har, rate, fmt, ch, x, n_frames, packets, tag):
    C_ = har.lib.stest_carry_len(rate)
    want = har.push(rate, fmt, ch, x, n_frames, packets, 0)
    got = har.push(rate, fmt, ch, x, n_frames, packets, 1)
    assert len(got) == len(want), tag
    ring = slice(G, G + RING)
    carry = slice(2 * G + RING, 2 * G + RING + C_)
    guards = [slice(0, G), slice(G + RING, 2 * G + RING), slice(2 * G + RING + C_, 3 * G + RING + C_), slice(3 * G + RING + 2 * C_, 4 * G + RING + 2 * C_)]
    for i in range(len(got)):
        assert got[i, ring].tobytes() == want[i, ring].tobytes(), (tag, "ring image", i)
        assert got[i, carry].tobytes() == want[i, carry].tobytes(), (tag, "carry image", i)
        for g in guards:
            assert np.all(np.isnan(got[i, g])), (tag, "a guard value changed in image", i)
    assert np.all(np.isfinite(want[:, ring])) and np.any(want[-1, ring] != 0)
    assert len(got) >= -(-(-(-n_frames * 16000 // rate)) // RING)       # the ring wrapped: 24 000 outputs through 4096 slots
    return len(got)


@pytest.mark.parametrize("fmt,ch", COMBOS)
@pytest.mark.parametrize("rate", RATES)
def test_push_is_the_restatement(har, tile, rate, fmt, ch):
    rng = np.random.default_rng(rate * 10 + fmt * 2 + ch)
    n_frames = rate * 3 // 2
    x = random_input(rng, n_frames, ch, fmt)
    for name, packets in splits_of(rate, n_frames, tile, rng).items():
        n = check_images(har, rate, fmt, ch, x, n_frames, packets, (rate, fmt, ch, name))
        assert n >= 6


@pytest.mark.parametrize("rate", RATES)
def test_push_extremes(har, tile, rate):
    n_frames = rate * 3 // 2
    rng = np.random.default_rng(rate)
    packets = splits_of(rate, n_frames, tile, rng)
    for fmt, ch in ((I16, 2), (F32, 1)):
        for name, x in (("square", square_input(n_frames, ch, fmt)), ("impulse", impulse_input(n_frames, ch, fmt, 997))):
            for split in ("irregular", "tile"):
                check_images(har, rate, fmt, ch, x, n_frames, packets[split], (rate, fmt, ch, name, split))


def window_specs(tile, cap):
    specs = []
    k = 0
    for length in (1, tile - 1, tile, tile + 1, 51200):
        shapes = {"plain": [(100, length)], "slot0": [(0, length)], "last": [(cap - length, length)]}
        if length >= 2:
            a = max(1, length // 3)
            shapes["wrap"] = [(cap - a, a), (0, length - a)]
            shapes["two"] = [(cap // 2 + 1, a), (7, length - a)]
        if length >= 8:
            a, b, c = 3, length // 2 - 3, 5
            shapes["four"] = [(cap - a, a), (0, b), (cap - c, c), (0, length - a - b - c)]
        for name, pieces in shapes.items():
            for src_off in range(4):
                for dst_off in range(4):
                    if length == 51200 and (src_off + dst_off + k) % 4:        # a quarter of the offset pairs at the long length: every offset still occurs on both sides
                        continue
                    specs.append((pieces, src_off, dst_off))
            k += 1
    return specs


@pytest.mark.parametrize("n_sessions", [1, 3, 8])
def test_window_gather(har, tile, n_sessions):
    cap = 60001
    rng = np.random.default_rng(n_sessions)
    ring = rng.uniform(-1.0, 1.0, cap).astype(np.float32)
    ring[:3] = [np.float32(-0.0), np.float32(1e-42), np.float32(np.inf)]                 # copied as bits: a negative zero, a subnormal, an infinity
    specs = window_specs(tile, cap)
    rng.shuffle(specs)
    assert len(specs) > 300
    for i0 in range(0, len(specs), n_sessions):
        grp = specs[i0:i0 + n_sessions]
        if len(grp) < n_sessions:
            grp = grp + specs[:n_sessions - len(grp)]
        got = har.window(ring, grp, 1)
        host = har.window(ring, grp, 0)
        for i, (pieces, src_off, dst_off) in enumerate(grp):
            want = np.concatenate([ring[s:s + l] for s, l in pieces])
            lo = G + dst_off
            assert got[i, lo:lo + len(want)].tobytes() == want.tobytes(), (pieces, src_off, dst_off)
            assert np.all(np.isnan(got[i, :lo])) and np.all(np.isnan(got[i, lo + len(want):])), ("a write outside the window", pieces, src_off, dst_off)
            assert host[i, lo:lo + len(want)].tobytes() == want.tobytes()

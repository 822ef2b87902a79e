"""The model loader's unpack kernels (whisper-rust_amd/csrc/wa_load.hip) one by one, BIT FOR BIT against the host functions that define the
arena layouts and that the loader's host path runs: wa_q32_unpack_rows (wa_quant1.h), wa_qk_unpack_rows (wa_quantk.h), wa_conv_reorder_rows
(wa_load.h), reached through tests/native/libload_ref.so.  The kernels are called through tests/native/libload_kernels.so, which
whisper-rust_amd/Makefile (target load_harness) links against the product's own build/wa_load.o.

Inputs are raw block bytes.  Dictated blocks: for the 32-value formats qh = 0, 0xffffffff and every single bit, all nibbles 0 and all 15,
Q8_0 quants -128 and 127, and d / m of the bit patterns 0x0000, 0x8000, 0x0001 (subnormal), 0x03ff, 0x7bff, 0xfbff; for the K formats every
6-bit scale and minimum value in every position of Q5_K's and Q3_K's packed scale bytes, the high-bit bytes of Q3_K, Q5_K and Q6_K all zero
and all one, Q2_K scale bytes 0x00, 0xff, 0x0f, 0xf0.  Then seeded random bytes with d / dmin drawn from the finite F16 patterns only (a
quantiser writes no infinite or NaN scale, and the payload of a converted NaN is not part of the contract).  Shapes: 3 rows x {1, 4, 6}
blocks of 32 (6: the row length 192 whose lane bytes are not 16-byte aligned), 2 rows x {1, 3} blocks of 256; conv re-order with IC 80 and
128, OC 3 and a padded row stride, and two shapes only the one-element kernel takes.  Every output goes into a sentinel-filled buffer one
row longer than written; the sentinel must survive there and in the padding."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "native", "libload_kernels.so")
REF_PATH = os.path.join(ROOT, "tests", "native", "libload_ref.so")
Q5_0, Q8_0, Q4_1, Q5_1, Q2_K, Q3_K, Q5_K, Q6_K = 6, 8, 3, 7, 10, 11, 13, 14
BYTES = {Q5_0: 22, Q8_0: 34, Q4_1: 20, Q5_1: 24, Q2_K: 84, Q3_K: 110, Q5_K: 176, Q6_K: 210}
NAME = {Q5_0: "q5_0", Q8_0: "q8_0", Q4_1: "q4_1", Q5_1: "q5_1", Q2_K: "q2_k", Q3_K: "q3_k", Q5_K: "q5_k", Q6_K: "q6_k"}
HAS_MIN = {Q4_1, Q5_1, Q2_K, Q5_K}
D_AT = {Q5_0: 0, Q8_0: 0, Q4_1: 0, Q5_1: 0, Q2_K: 80, Q3_K: 108, Q5_K: 0, Q6_K: 208}       # where the block keeps d (dmin / m follows it)
F16_PATTERNS = (0x0000, 0x8000, 0x0001, 0x03ff, 0x7bff, 0xfbff)
SENT8, SENT16, SENT32 = 0x80, 0x7E5A, 0x7FC0DEAD      # -128 is no K or 5-bit quant; where a Q8_0 quant may be -128 the comparison with the reference decides
vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t


@functools.lru_cache(maxsize=None)
def lib():
    assert os.path.exists(LIB_PATH), "%s missing: build() makes it (whisper-rust_amd/Makefile, target load_harness)" % LIB_PATH
    L = C.CDLL(LIB_PATH)
    L.ltest_alloc.restype = vp; L.ltest_alloc.argtypes = [sz]
    L.ltest_free.argtypes = [vp]
    L.ltest_h2d.argtypes = [vp, vp, sz]; L.ltest_d2h.argtypes = [vp, vp, sz]
    L.ltest_load_q32.argtypes = [ci, vp, sz, sz, vp, vp, vp]
    L.ltest_load_qk.argtypes = [ci, vp, sz, sz, vp, vp, vp, vp]
    L.ltest_load_conv.argtypes = [vp, sz, ci, ci, vp, vp]
    return L


@functools.lru_cache(maxsize=None)
def ref():
    assert os.path.exists(REF_PATH), "%s missing: build() makes it" % REF_PATH
    R = C.CDLL(REF_PATH)
    R.lref_q32.argtypes = [ci, vp, sz, sz, vp, vp, vp]; R.lref_q32.restype = None
    R.lref_qk.argtypes = [ci, vp, sz, sz, vp, vp, vp, vp]; R.lref_qk.restype = None
    R.lref_conv.argtypes = [vp, sz, ci, ci, vp, vp]; R.lref_conv.restype = None
    R.lref_q32_block.argtypes = [ci, vp, vp, vp, vp]; R.lref_q32_block.restype = None
    R.lref_qk_block.argtypes = [ci, vp, vp, vp, vp, vp]; R.lref_qk_block.restype = None
    return R


class Dev:
    """Device copies of host arrays; everything allocated through one Dev is freed by close()."""

    def __init__(self):
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = lib().ltest_alloc(max(a.nbytes, 16))
        assert p, "device allocation of %d bytes failed" % a.nbytes
        self.bufs.append(p)
        assert lib().ltest_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    @staticmethod
    def get(p, like):
        out = np.empty_like(like)
        assert lib().ltest_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.bufs:
            lib().ltest_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def assert_bits(got, want, what):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %#x want %#x" % (what, bad.size, want.size, bad[0], int(got[bad[0]]), int(want[bad[0]]))


def put16(blk, at, h):
    blk[at], blk[at + 1] = h & 0xff, h >> 8


def finite_f16(rng, n):
    h = rng.integers(0, 65536, size=n, dtype=np.uint32)
    while True:
        bad = ((h >> 10) & 31) == 31
        if not bad.any():
            return h
        h[bad] = rng.integers(0, 65536, size=int(bad.sum()), dtype=np.uint32)


# ----------------------------------------------------------------------------------------------------------------------------
# blocks (made once per format, shared by the tests, never changed)
# ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dictated_q32(t):
    rng = np.random.default_rng(100 + t)
    out = []

    def block(qs, qh=None):
        b = np.zeros(BYTES[t], dtype=np.uint8)
        k = len(out)
        put16(b, 0, F16_PATTERNS[k % 6])
        at = 2
        if t in HAS_MIN:
            put16(b, 2, F16_PATTERNS[(k // 6 + k) % 6]); at = 4
        if t in (Q5_0, Q5_1):
            b[at:at + 4] = np.frombuffer(np.uint32(qh).tobytes(), dtype=np.uint8); at += 4
        b[at:] = qs
        out.append(b)

    if t == Q8_0:
        for fill in (0x80, 0x7f):
            for _ in range(6):
                block(np.full(32, fill, dtype=np.uint8))
        for _ in range(6):
            block(np.tile(np.array([0x80, 0x7f, 0x00, 0xff], dtype=np.uint8), 8))
        return out
    if t == Q4_1:
        for fill in (0x00, 0xff, 0x0f, 0xf0):
            for _ in range(9):
                block(np.full(16, fill, dtype=np.uint8))
        return out
    for qh in [0, 0xffffffff] + [1 << j for j in range(32)]:
        block(rng.integers(0, 256, size=16, dtype=np.uint8), qh)
    for fill in (0x00, 0xff):
        for qh in (0, 0xffffffff, 0x0000ffff, 0xffff0000):
            block(np.full(16, fill, dtype=np.uint8), qh)
    return out


def pack_q5k_scales(sc, m):
    s = np.zeros(12, dtype=np.uint8)
    for j in range(4):
        s[j] = sc[j] | ((sc[j + 4] >> 4) << 6)
        s[j + 4] = m[j] | ((m[j + 4] >> 4) << 6)
        s[j + 8] = (sc[j + 4] & 0xf) | ((m[j + 4] & 0xf) << 4)
    return s


def pack_q3k_scales(raw):          # raw[k] = the 6-bit field of sub-block k, 0..63 (the scale is raw - 32)
    s = np.zeros(12, dtype=np.uint8)
    for k in range(8):
        s[k] = (raw[k] & 0xf) | ((raw[k + 8] & 0xf) << 4)
    for i in range(4):
        s[8 + i] = sum(((raw[i + 4 * q] >> 4) & 3) << (2 * q) for q in range(4))
    return s


def q5k_fields(k):
    return [(k + 5 * j) % 64 for j in range(8)], [(3 * k + 7 * j + 11) % 64 for j in range(8)]


def q3k_fields(k):
    return [(k + 5 * p) % 64 for p in range(16)]


@functools.lru_cache(maxsize=None)
def dictated_qk(t):
    rng = np.random.default_rng(200 + t)
    out = []

    def block(edit):
        b = rng.integers(0, 256, size=BYTES[t], dtype=np.uint8)
        k = len(out)
        put16(b, D_AT[t], F16_PATTERNS[k % 6])
        if t in HAS_MIN:
            put16(b, D_AT[t] + 2, F16_PATTERNS[(k // 6 + k) % 6])
        edit(b)
        out.append(b)

    def setb(lo, hi, v):
        def f(b):
            b[lo:hi] = v
        return f

    if t == Q5_K:       # d, dmin, scales[12] at 4, qh[32] at 16, qs[128] at 48
        for k in range(64):
            block(setb(4, 16, pack_q5k_scales(*q5k_fields(k))))
        block(setb(16, 48, 0x00)); block(setb(16, 48, 0xff))
    elif t == Q3_K:     # hmask[32], qs[64] at 32, scales[12] at 96, d at 108
        for k in range(64):
            block(setb(96, 108, pack_q3k_scales(q3k_fields(k))))
        block(setb(0, 32, 0x00)); block(setb(0, 32, 0xff))
    elif t == Q6_K:     # ql[128], qh[64] at 128, scales[16] at 192, d at 208
        block(setb(128, 192, 0x00)); block(setb(128, 192, 0xff))
        block(setb(0, 128, 0x00)); block(setb(0, 128, 0xff))
        block(setb(192, 208, 0x80)); block(setb(192, 208, 0x7f))
    else:               # Q2_K: scales[16], qs[64] at 16, d at 80, dmin at 82
        for v in (0x00, 0xff, 0x0f, 0xf0):
            block(setb(0, 16, v))
        block(setb(16, 80, 0x00)); block(setb(16, 80, 0xff))
    return out


def tensors_of(blocks, rows, nb):
    """the dictated blocks dealt over as many [rows][nb] tensors as it takes (the last one wraps round to the first blocks)"""
    per = rows * nb
    n = (len(blocks) + per - 1) // per
    return [np.stack([blocks[(i * per + j) % len(blocks)] for j in range(per)]).reshape(rows, nb, -1) for i in range(n)]


@functools.lru_cache(maxsize=None)
def random_tensor(t, rows, nb):
    rng = np.random.default_rng(1000 * t + 10 * rows + nb)
    a = rng.integers(0, 256, size=(rows, nb, BYTES[t]), dtype=np.uint8)
    for at in (D_AT[t],) + ((D_AT[t] + 2,) if t in HAS_MIN else ()):
        h = finite_f16(rng, rows * nb).reshape(rows, nb)
        a[:, :, at] = h & 0xff
        a[:, :, at + 1] = h >> 8
    a.setflags(write=False)
    return a


# ----------------------------------------------------------------------------------------------------------------------------
# one launch against the host function
# ----------------------------------------------------------------------------------------------------------------------------
def check_q32(dev, t, src, what):
    rows, nb = src.shape[:2]
    qs = np.full((rows + 1) * nb * 32, SENT8, dtype=np.uint8)
    qd = np.full((rows + 1) * nb, SENT32, dtype=np.uint32)
    qm = np.full((rows + 1) * nb, SENT32, dtype=np.uint32)
    mn = t in HAS_MIN
    want = [qs.copy(), qd.copy(), qm.copy()]
    ref().lref_q32(t, src.ctypes.data, rows, nb, want[0].ctypes.data, want[1].ctypes.data, want[2].ctypes.data if mn else None)
    d = [dev.put(qs), dev.put(qd), dev.put(qm)]
    assert lib().ltest_load_q32(t, dev.put(src), rows, nb, d[0], d[1], d[2] if mn else None) == 0
    assert lib().ltest_sync() == 0
    got = [Dev.get(d[0], qs), Dev.get(d[1], qd), Dev.get(d[2], qm)]
    for g, w, n in zip(got, want, ("quants", "scales", "minimums")):
        assert_bits(g, w, "%s %s %s" % (NAME[t], what, n))
    assert (got[0][rows * nb * 32:] == SENT8).all() and (got[1][rows * nb:] == SENT32).all() and (got[2][(rows * nb if mn else 0):] == SENT32).all()
    assert (want[1][:rows * nb] != SENT32).all()          # the reference did write: the comparison is not sentinel against sentinel


def check_qk(dev, t, src, what):
    rows, nb = src.shape[:2]
    qs = np.full((rows + 1) * nb * 256, SENT8, dtype=np.uint8)
    qsc = np.full((rows + 1) * nb * 16, SENT8, dtype=np.uint8)
    qd = np.full((rows + 1) * nb, SENT32, dtype=np.uint32)
    qm = np.full((rows + 1) * nb, SENT32, dtype=np.uint32)
    mn = t in HAS_MIN
    want = [qs.copy(), qsc.copy(), qd.copy(), qm.copy()]
    ref().lref_qk(t, src.ctypes.data, rows, nb, want[0].ctypes.data, want[1].ctypes.data, want[2].ctypes.data, want[3].ctypes.data if mn else None)
    d = [dev.put(qs), dev.put(qsc), dev.put(qd), dev.put(qm)]
    assert lib().ltest_load_qk(t, dev.put(src), rows, nb, d[0], d[1], d[2], d[3] if mn else None) == 0
    assert lib().ltest_sync() == 0
    got = [Dev.get(d[0], qs), Dev.get(d[1], qsc), Dev.get(d[2], qd), Dev.get(d[3], qm)]
    for g, w, n in zip(got, want, ("quants", "scale bytes", "d", "dmin")):
        assert_bits(g, w, "%s %s %s" % (NAME[t], what, n))
    assert (got[0][rows * nb * 256:] == SENT8).all() and (got[1][rows * nb * 16:] == SENT8).all() and (got[2][rows * nb:] == SENT32).all()
    assert (got[3][(rows * nb if mn else 0):] == SENT32).all()
    assert (want[2][:rows * nb] != SENT32).all() and (want[0][:rows * nb * 256] != SENT8).all()


# ----------------------------------------------------------------------------------------------------------------------------
# the cases say what they claim (no device)
# ----------------------------------------------------------------------------------------------------------------------------
def unpack_q32_block(t, b):
    q, d, m = np.zeros(32, dtype=np.int8), C.c_float(), C.c_float()
    ref().lref_q32_block(t, b.ctypes.data, q.ctypes.data, C.byref(d), C.byref(m))
    return q


def unpack_qk_block(t, b):
    q, sc, d, m = np.zeros(256, dtype=np.int8), np.zeros(16, dtype=np.int8), C.c_float(), C.c_float()
    ref().lref_qk_block(t, b.ctypes.data, q.ctypes.data, sc.ctypes.data, C.byref(d), C.byref(m))
    return q, sc


def test_dictated_blocks_reach_what_they_name():
    lo_hi = {Q5_0: (-16, 15), Q5_1: (0, 31), Q4_1: (0, 15), Q8_0: (-128, 127)}
    for t, (lo, hi) in lo_hi.items():
        qs = np.concatenate([unpack_q32_block(t, b) for b in dictated_q32(t)])
        assert qs.min() == lo and qs.max() == hi, NAME[t]
        heads = {(int(b[0]) | int(b[1]) << 8) for b in dictated_q32(t)}
        assert heads == set(F16_PATTERNS)
        if t in HAS_MIN:
            assert {(int(b[2]) | int(b[3]) << 8) for b in dictated_q32(t)} == set(F16_PATTERNS)
    # Q5_K: every value 0..63 as scale and as minimum of every sub-block, the fields as intended (the packing above is the inverse of get_scale_min_k4)
    seen_sc, seen_m = [set() for _ in range(8)], [set() for _ in range(8)]
    for k in range(64):
        _, sc = unpack_qk_block(Q5_K, dictated_qk(Q5_K)[k])
        want_sc, want_m = q5k_fields(k)
        assert sc[:8].tolist() == want_sc and sc[8:].tolist() == want_m
        for j in range(8):
            seen_sc[j].add(int(sc[j])); seen_m[j].add(int(sc[8 + j]))
    assert all(s == set(range(64)) for s in seen_sc + seen_m)
    # Q3_K: every 6-bit field value in each of the 16 positions; the unpacked scale of sub-block k sits at 8 (k & 1) + (k >> 1)
    seen = [set() for _ in range(16)]
    for k in range(64):
        _, sc = unpack_qk_block(Q3_K, dictated_qk(Q3_K)[k])
        raw = q3k_fields(k)
        assert [int(sc[8 * (p & 1) + (p >> 1)]) for p in range(16)] == [r - 32 for r in raw]
        for p in range(16):
            seen[p].add(raw[p])
    assert all(s == set(range(64)) for s in seen)
    q0, _ = unpack_qk_block(Q3_K, dictated_qk(Q3_K)[64]); q1, _ = unpack_qk_block(Q3_K, dictated_qk(Q3_K)[65])
    assert q0.max() <= -1 and q1.min() >= 0               # mask all zero: every value minus 4; all one: none
    q0, _ = unpack_qk_block(Q6_K, dictated_qk(Q6_K)[0]); q1, _ = unpack_qk_block(Q6_K, dictated_qk(Q6_K)[1])
    assert q0.max() <= -17 and q1.min() >= 16
    q0, _ = unpack_qk_block(Q5_K, dictated_qk(Q5_K)[64]); q1, _ = unpack_qk_block(Q5_K, dictated_qk(Q5_K)[65])
    assert q0.max() <= 15 and q1.min() >= 16
    assert [int(unpack_qk_block(Q2_K, dictated_qk(Q2_K)[i])[1][0]) & 0xff for i in range(4)] == [0x00, 0xff, 0x0f, 0xf0]


# ----------------------------------------------------------------------------------------------------------------------------
# the kernels
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 4, 6])
@pytest.mark.parametrize("t", [Q5_0, Q8_0, Q5_1, Q4_1], ids=lambda t: NAME[t])
def test_q32_dictated_blocks(dev, t, nb):
    for i, src in enumerate(tensors_of(dictated_q32(t), 3, nb)):
        check_q32(dev, t, src, "dictated tensor %d, %d blocks a row" % (i, nb))
        dev.close()


@pytest.mark.parametrize("nb", [1, 4, 6])
@pytest.mark.parametrize("t", [Q5_0, Q8_0, Q5_1, Q4_1], ids=lambda t: NAME[t])
def test_q32_random_bytes(dev, t, nb):
    check_q32(dev, t, random_tensor(t, 3, nb), "random, %d blocks a row" % nb)


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("t", [Q2_K, Q3_K, Q5_K, Q6_K], ids=lambda t: NAME[t])
def test_qk_dictated_blocks(dev, t, nb):
    for i, src in enumerate(tensors_of(dictated_qk(t), 2, nb)):
        check_qk(dev, t, src, "dictated tensor %d, %d blocks a row" % (i, nb))
        dev.close()


@pytest.mark.parametrize("nb", [1, 3])
@pytest.mark.parametrize("t", [Q2_K, Q3_K, Q5_K, Q6_K], ids=lambda t: NAME[t])
def test_qk_random_bytes(dev, t, nb):
    check_qk(dev, t, random_tensor(t, 2, nb), "random, %d blocks a row" % nb)


def test_q32_more_than_one_workgroup(dev):
    """40 rows of 40 blocks (d = 1280): 3200 threads, 13 workgroups of the 16-byte kernel"""
    check_q32(dev, Q5_1, random_tensor(Q5_1, 40, 40), "random, 40 x 40")


def test_qk_more_than_one_workgroup(dev):
    check_qk(dev, Q3_K, random_tensor(Q3_K, 33, 5), "random, 33 x 5")


# IC 80 / 128 with a padded stride: the eight-channel kernel; IC 12, and a stride that is no multiple of 8: the one-element kernel
@pytest.mark.parametrize("IC,ld", [(80, 256), (128, 3 * 128 + 16), (12, 40), (80, 243)])
def test_conv_reorder(dev, IC, ld):
    OC = 3
    rng = np.random.default_rng(IC * 1000 + ld)
    src = rng.integers(0, 65536, size=OC * IC * 3, dtype=np.uint16)
    dst = np.full((OC + 1) * ld, SENT16, dtype=np.uint16)
    cp = np.full((OC + 1) * IC * 3, SENT16, dtype=np.uint16)
    want_dst, want_cp = dst.copy(), cp.copy()
    ref().lref_conv(src.ctypes.data, OC, IC, ld, want_dst.ctypes.data, want_cp.ctypes.data)
    # the host function against the plain statement of the re-order: [oc][ic][k] -> [oc][k][ic]
    assert np.array_equal(want_dst.reshape(OC + 1, ld)[:OC, :3 * IC].reshape(OC, 3, IC), src.reshape(OC, IC, 3).transpose(0, 2, 1))
    d_dst, d_cp = dev.put(dst), dev.put(cp)
    assert lib().ltest_load_conv(dev.put(src), OC, IC, ld, d_dst, d_cp) == 0
    assert lib().ltest_sync() == 0
    got_dst, got_cp = Dev.get(d_dst, dst), Dev.get(d_cp, cp)
    assert_bits(got_dst, want_dst, "re-ordered rows")
    assert_bits(got_cp, want_cp, "copy")
    assert (got_dst.reshape(OC + 1, ld)[:, 3 * IC:] == SENT16).all() and (got_dst[OC * ld:] == SENT16).all() and (got_cp[OC * IC * 3:] == SENT16).all()
    assert np.array_equal(got_cp[:OC * IC * 3], src)


def test_launchers_refuse_what_they_cannot_place(dev):
    """a null array, a minimum array for a format without one, an unknown type: an error code and no launch"""
    src = random_tensor(Q5_0, 3, 4)
    qs, qd = dev.put(np.zeros(4 * 4 * 32, dtype=np.uint8)), dev.put(np.zeros(16, dtype=np.float32))
    assert lib().ltest_load_q32(Q5_0, dev.put(src), 3, 4, qs, qd, qd) != 0
    assert lib().ltest_load_q32(Q5_1, dev.put(src), 3, 4, qs, qd, None) != 0
    assert lib().ltest_load_q32(2, dev.put(src), 3, 4, qs, qd, None) != 0
    assert lib().ltest_load_qk(Q6_K, dev.put(src), 1, 1, qs, None, qd, None) != 0
    assert lib().ltest_load_conv(dev.put(src), 1, 8, 16, qs, qs) != 0          # a stride shorter than a row
    assert lib().ltest_sync() == 0

"""The kernels of wa_quant.hip one by one - the Q8_0 / Q8_1 quantiser, the one-row and the 8-row product of every format family with
every epilogue, the fused GELU product, the quantised token embedding - against the host reference, BIT FOR BIT (NaN equals NaN).

The cases and their expected values come from tools/quant_cases.py: operands dictated rather than quantised (scales of both signs
binades apart, subnormal halfs, zeros, Q8_0 bytes of -128, saturated rows, block sums of +-inf), quantiser rows on the rounding points
(ties of rint, id = 0, a negative maximum, s at and beyond the F16 limit, d a subnormal half or an F16 infinity), block counts that take
every clamp and guard of the pipelined loop and the block-by-block loop, partial tiles in both directions, and K = 5120 with a
minimum, which takes the raised-LDS-limit branch of the launcher.  tests/test_quant_kernels_math.py shows on the CPU that a kernel
with a different summation order, a split fmaf, a fused or shortened minimum chain or another rounding in the quantiser would change
these expected values.

The kernels are called through tests/native/libquant_kernels.so, which oracle/Makefile links against the product's own
whisper-rust_amd/build/wa_quant.o (WA_QTEST_LIB names another build of it).  Every output buffer is filled with a sentinel first;
padding (ldx > K, ldo > N, rows beyond M) must still hold it afterwards.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import quant_cases as QC  # noqa: E402

LIB_PATH = os.environ.get("WA_QTEST_LIB") or os.path.join(ROOT, "tests", "native", "libquant_kernels.so")
SENT8 = np.int8(-128)         # sentinels: bit patterns no kernel result can have (a Q8 quant is -127 .. 127, the others are NaNs with a payload)
SENT16 = np.uint16(0x7E5A)
SENT32 = np.uint32(0x7FC0DEAD)


class QtEpi(C.Structure):      # tests/native/quant_kernels.hip: qtest_epi
    _fields_ = [("bias", C.c_void_p), ("scale", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int), ("out2", C.c_void_p), ("ldo2", C.c_int),
                ("out3", C.c_void_p), ("ldo3", C.c_int), ("resid", C.c_void_p), ("ldr", C.c_int), ("gelu", C.c_void_p),
                ("split0", C.c_int), ("split1", C.c_int), ("row_off", C.c_int), ("aux0", C.c_int), ("aux1", C.c_int)]


_LIB = None


def lib():
    global _LIB
    if _LIB is None:
        assert os.path.exists(LIB_PATH), "%s missing: build() makes it (oracle/Makefile, target harness)" % LIB_PATH
        L = C.CDLL(LIB_PATH)
        vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
        L.qtest_alloc.restype = vp; L.qtest_alloc.argtypes = [sz]
        L.qtest_free.argtypes = [vp]
        L.qtest_h2d.argtypes = [vp, vp, sz]; L.qtest_d2h.argtypes = [vp, vp, sz]
        L.qtest_quantize_q8_0.argtypes = [vp, i, i, i, vp, vp, vp]
        L.qtest_qgemm_exact.argtypes = [i, vp, vp, i, vp, vp, i, i, C.POINTER(QtEpi), vp, vp]
        L.qtest_qgemv_gelu_q8.argtypes = [vp, vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp]
        L.qtest_dec_embed_q.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp]
        _LIB = L
    return _LIB


class Dev:
    """Device copies of host arrays; everything allocated through one Dev is freed by close()."""

    def __init__(self):
        self.bufs = []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = lib().qtest_alloc(max(a.nbytes, 16))
        assert p, "device allocation of %d bytes failed" % a.nbytes
        self.bufs.append(p)
        assert lib().qtest_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    @staticmethod
    def get(p, like):
        out = np.empty_like(like)
        assert lib().qtest_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def close(self):
        for p in self.bufs:
            lib().qtest_free(p)
        self.bufs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.close()


def sync():
    err = lib().qtest_sync()
    assert err == 0, "HIP error %d after the launch" % err


def assert_bits(got, want, what):
    """Integer arrays (quants, F16 bits): equal."""
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %#x want %#x" % (what, bad.size, want.size, bad[0], int(got[bad[0]]) & 0xffffffff,
                                                                                   int(want[bad[0]]) & 0xffffffff)


def assert_f32(got, want, what):
    """F32 bits as uint32: equal, except that any NaN but the sentinel stands for an expected NaN."""
    got, want = np.asarray(got, np.uint32).ravel(), np.asarray(want, np.uint32).ravel()
    want_nan = np.isnan(want.view(np.float32)) & (want != SENT32)
    ok = np.where(want_nan, np.isnan(got.view(np.float32)) & (got != SENT32), got == want)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %#x (%r) want %#x (%r)" % (
        what, bad.size, want.size, bad[0], got[bad[0]], got.view(np.float32)[bad[0]], want[bad[0]], want.view(np.float32)[bad[0]])


def put_weights(dev, w):
    return dev.put(QC.pack_qs(w["q"])), dev.put(w["d"]), (dev.put(w["m"]) if w["m"] is not None else None)


def put_activations(dev, x, q1):
    return dev.put(QC.pack_qs(x["q"])), dev.put(x["d"]), (dev.put(x["s"]) if q1 else None)


# ----------------------------------------------------------------------------------------------------------------------------
# k_quantize_q8_0
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_qsum", (True, False), ids=("q8_1", "q8_0"))
@pytest.mark.parametrize("c", QC.QUANT_CASES, ids=[c["name"] for c in QC.QUANT_CASES])
def test_quantize(dev, c, with_qsum):
    """Rows with a stride ldx = K + 8 (the padding holds values far larger than the rows': reading it would change a block's maximum).
    3 x 96 and 5 x 160 end in a workgroup whose last wave has one active half.  Without qsum that buffer keeps its sentinel."""
    rows, K, ldx = c["rows"], c["K"], c["ldx"]
    nb = K // 32
    X, _ = QC.quant_rows(c)
    Xp = np.full((rows, ldx), 3e38, np.float32)
    Xp[:, :K] = X
    q, d, s = QC.ref_quantize(X)
    sent_s = np.full((rows, nb), SENT32, np.uint32)
    p_qs, p_qd, p_s = dev.put(np.full((rows, 8, nb, 4), SENT8, np.int8)), dev.put(np.full((rows, nb), SENT32, np.uint32)), dev.put(sent_s)
    lib().qtest_quantize_q8_0(dev.put(Xp), ldx, rows, K, p_qs, p_qd, p_s if with_qsum else None)
    sync()
    assert_bits(Dev.get(p_qs, QC.pack_qs(q)), QC.pack_qs(q), "quants")
    assert_f32(Dev.get(p_qd, sent_s), QC.bits32(d), "d")
    assert_f32(Dev.get(p_s, sent_s), QC.bits32(s) if with_qsum else sent_s, "s")


# ----------------------------------------------------------------------------------------------------------------------------
# the products, WA_EPI_F32 without bias
# ----------------------------------------------------------------------------------------------------------------------------
def run_product_f32(dev, c):
    M, N, K = c["M"], c["N"], c["nb"] * 32
    w, x = QC.product_operands(c)
    q1 = w["m"] is not None
    ldo = N + 3
    want = np.full((M + 1, ldo), SENT32, np.uint32)            # one row beyond M
    want[:M, :N] = QC.bits32(QC.ref_gemm(w, x))
    p_out = dev.put(np.full((M + 1, ldo), SENT32, np.uint32))
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, q1)
    e = QtEpi(out=p_out, ldo=ldo)
    lib().qtest_qgemm_exact(QC.F32, xq, xd, M, wq, wd, N, K, C.byref(e), xs, wm)
    sync()
    assert_f32(Dev.get(p_out, want), want, c["name"] + " (" + c["kind"] + ")")


GEMV_KEYS = sorted({(c["fmt"], c["nb"]) for c in QC.GEMV_CASES})


@pytest.mark.parametrize("fmt,nb", GEMV_KEYS, ids=["%s_nb%d" % k for k in GEMV_KEYS])
def test_one_row_product(dev, fmt, nb):
    """k_qgemv_exact at N = 1, 7, 8, 13, 40 (fewer rows than a workgroup's 8, a partial last workgroup): nb = 1, 2, 3, 5, 6 take the
    block-by-block loop, nb = 4 .. 96 the pipelined one with its clamped prefetches and the guard of a partial last round."""
    cases = [c for c in QC.GEMV_CASES if (c["fmt"], c["nb"]) == (fmt, nb)]
    assert [c["N"] for c in cases] == list(QC.GEMV_N)
    for c in cases:
        run_product_f32(dev, c)


GEMM_KEYS = sorted({(QC.family(c["fmt"]), c["nb"], c["M"]) for c in QC.GEMM_CASES})


@pytest.mark.parametrize("fam,nb,M", GEMM_KEYS, ids=["%s_nb%d_M%d" % k for k in GEMM_KEYS])
def test_eight_row_product(dev, fam, nb, M):
    """k_qgemm_exact at N = 5, 32, 33, 70: M = 2 and the last tiles of M = 9, 17 hold fewer than 8 rows, M = 9, 17 have grid.y > 1; with
    a minimum, M = 8 and 9 hand over the chain of every lane."""
    cases = [c for c in QC.GEMM_CASES if (QC.family(c["fmt"]), c["nb"], c["M"]) == (fam, nb, M)]
    assert [c["N"] for c in cases] == list(QC.GEMM_N)
    for c in cases:
        run_product_f32(dev, c)


@pytest.mark.parametrize("c", QC.GEMM_BIG_CASES, ids=[c["name"] for c in QC.GEMM_BIG_CASES])
def test_eight_row_product_k5120(dev, c):
    """K = 5120: with a minimum the activation tile is 51 200 B of LDS and the launcher raises the kernel's limit first; the Q8_0 twin
    needs 46 080 B and launches as it is."""
    lds = 8 * c["nb"] * 32 + (16 if QC.family(c["fmt"]) == "Q1" else 8) * c["nb"] * 4
    assert (lds > 48 * 1024) == (c["fmt"] == "q5_1")
    run_product_f32(dev, c)


# ----------------------------------------------------------------------------------------------------------------------------
# the epilogues
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", QC.EPI_CASES, ids=[c["name"] for c in QC.EPI_CASES])
def test_epilogue(dev, c):
    """M = 9 (k_qgemm_exact) and M = 1 (k_qgemv_exact), N = 70, K = 128: every value at the place the epilogue's index map gives it,
    everything else still the sentinel."""
    M, N, K = c["M"], c["N"], c["nb"] * 32
    w, x, ops = QC.epi_operands(c)
    q1 = w["m"] is not None
    bufs, fields = QC.epi_layout(c)
    val = QC.epi_expected(c)
    want = {name: np.full(n, SENT16 if t == "f16" else SENT32, np.uint16 if t == "f16" else np.uint32) for name, (n, t) in bufs.items()}
    m, n = np.meshgrid(np.arange(M), np.arange(N), indexing="ij")
    which, idx, names = QC.epi_out_index(c, fields, m, n)
    bits = val if val.dtype == np.uint16 else QC.bits32(val)
    for k, name in enumerate(names):
        sel = which == k
        assert np.unique(idx[sel]).size == np.count_nonzero(sel) and idx[sel].max() < want[name].size
        want[name][idx[sel]] = bits[sel]
    ptrs = {name: dev.put(np.full_like(a, SENT16 if a.dtype == np.uint16 else SENT32)) for name, a in want.items()}
    e = QtEpi(bias=dev.put(ops["bias"]) if ops["bias"] is not None else None, scale=dev.put(ops["scale"]) if ops["scale"] is not None else None,
              resid=dev.put(ops["resid"]) if ops["resid"] is not None else None, gelu=dev.put(QC.GELU) if c["epi"] == "GELU_F32" else None,
              out=ptrs["out"], out2=ptrs.get("out2"), out3=ptrs.get("out3"), **fields)
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, q1)
    lib().qtest_qgemm_exact(c["mode"], xq, xd, M, wq, wd, N, K, C.byref(e), xs, wm)
    sync()
    for name, a in want.items():
        got = Dev.get(ptrs[name], a)
        (assert_bits if a.dtype == np.uint16 else assert_f32)(got, a, c["name"] + " " + name)
    if c["epi"] == "GELU_F32":          # the edges came out as the table says
        rows = np.arange(3, 3 + 5 * len(QC.GELU_EDGES), 5)
        assert np.array_equal(QC.bits32(val[0, rows]), QC.bits32(QC.gelu32(np.float32(0) + np.array(QC.GELU_EDGES, np.float32))))


# ----------------------------------------------------------------------------------------------------------------------------
# k_qgemv_gelu_q8
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", QC.GELU_CASES, ids=[c["name"] for c in QC.GELU_CASES])
def test_fused_gelu_product(dev, c):
    """The first MLP product of a decode step: dot + bias, GELU, and the Q8_0 / Q8_1 row of the result, one output block per workgroup.
    The output blocks are all zero (every pre-activation <= -10), mixed with one pre-activation >= 10, or on ties of the quantiser.
    Without a minimum the block sums are not an output: their buffer is passed all the same and must keep its sentinel."""
    N, K = c["N"], c["nb"] * 32
    w, x, bias, _ = QC.gelu_operands(c)
    q1 = w["m"] is not None
    _, q, d, s = QC.gelu_expected(c)
    sent = np.full((1, N // 32), SENT32, np.uint32)
    p_oq, p_od, p_os = dev.put(np.full((1, 8, N // 32, 4), SENT8, np.int8)), dev.put(sent), dev.put(sent)
    wq, wd, wm = put_weights(dev, w)
    xq, xd, xs = put_activations(dev, x, q1)
    lib().qtest_qgemv_gelu_q8(xq, xd, wq, wd, N, K, dev.put(bias), dev.put(QC.GELU), p_oq, p_od, xs, wm, p_os)
    sync()
    assert_bits(Dev.get(p_oq, QC.pack_qs(q)), QC.pack_qs(q), "quants")
    assert_f32(Dev.get(p_od, sent), QC.bits32(d), "d")
    assert_f32(Dev.get(p_os, sent), QC.bits32(s) if q1 else sent, "s")


# ----------------------------------------------------------------------------------------------------------------------------
# k_dec_embed_q
# ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", QC.EMBED_CASES, ids=[c["name"] for c in QC.EMBED_CASES])
def test_token_embedding(dev, c):
    """Rows 0, 49 (the last) and repeats of a 50-row table at positions out of order: q * d, (+ m with a minimum,) + pe."""
    w, pe, tok, pos = QC.embed_operands(c)
    d = c["d"]
    want = np.full((tok.size + 1, d), SENT32, np.uint32)
    want[:tok.size] = QC.bits32(QC.embed_expected(c))
    p_x = dev.put(np.full_like(want, SENT32))
    wq, wd, wm = put_weights(dev, w)
    lib().qtest_dec_embed_q(dev.put(tok), dev.put(pos), tok.size, d, wq, wd, dev.put(pe), p_x, wm)
    sync()
    assert_f32(Dev.get(p_x, want), want, c["name"])
